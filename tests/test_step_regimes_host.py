"""The conditions under which tests/test_gpu_step_regimes.py says something, checked on the
step oracle alone.  No GPU.

Every regime of tests/_step_regimes.py must keep its population alive and busy for the six
steps, must make its parameter bind (a d_min nobody is clipped to tests nothing), and must
leave enough CLEAN steps - steps in which no decision of the oracle sits within a rounding
margin of flipping (_step_regimes.census) - for the device to be compared without excuses."""
from types import SimpleNamespace

import numpy as np
import pytest

import _step_regimes as R

SEXED = [n for n in R.NAMES if R.CASES[n][0].get('sexed')]


@pytest.mark.parametrize('name', R.NAMES)
def test_regime_is_lively(name):
    """each of the 6 steps starts with N >= 40 and has at least one pair, birth and death"""
    recs = R.oracle_run(name)
    assert len(recs) == R.N_STEPS
    for t, r in enumerate(recs):
        assert r['N0'] >= 40 and r['pairs'] >= 1 and r['births'] >= 1 and r['deaths'] >= 1, \
            (name, t, r['N0'], r['pairs'], r['births'], r['deaths'])


def test_d_min_binds():
    for t, r in enumerate(R.oracle_run('d_min')):
        assert r['n_d_min'] >= 100, (t, r['n_d_min'])


def test_d_max_binds():
    n = [r['n_d_max'] for r in R.oracle_run('d_max')]
    assert sum(k >= 5 for k in n) >= 4, n


def test_max_age_binds():
    for t, r in enumerate(R.oracle_run('max_age')):
        assert r['n_older_3'] >= 20, (t, r['n_older_3'])


def test_K_layer_zero_binds():
    for t, r in enumerate(R.oracle_run('K_layer_zero')):
        assert r['n_on_K0'] >= 5, (t, r['n_on_K0'])


def test_repro_age_binds():
    """fewer pairs in the first step than the default has"""
    a, b = R.oracle_run('repro_age')[0]['pairs'], R.oracle_run('default')[0]['pairs']
    print('pairs in step 1: repro_age %d, default %d' % (a, b))
    assert a < b, (a, b)


@pytest.mark.parametrize('name', ['births_poisson', 'sexed_ages'])
def test_poisson_births_bind(name):
    """the Poisson counts vary and the clip at one binds: some pair whose draw was raised to
    the minimum of 1 - the reference clips its Poisson draws at 1 (ops/mating.py:124-125), and
    so do gnx_draws.births_draws and the device, so no pair ever has 0 births - and some pair
    with 2 or more"""
    nb = np.concatenate([r['births_per_pair'] for r in R.oracle_run(name)])
    assert nb.min() == 1 and (nb >= 2).any(), np.bincount(nb)


@pytest.mark.parametrize('name', SEXED)
def test_sexed_regimes_bind(name):
    """both sexes present in every step, the focal individuals all female, the mates all male"""
    assert len(SEXED) == 4
    for t, r in enumerate(R.oracle_run(name)):
        assert r['n_male'] >= 1 and r['n_female'] >= 1, (name, t, r['n_male'], r['n_female'])
        assert (r['focal_sex'] == 0).all() and (r['mate_sex'] == 1).all(), (name, t)


def test_births_fixed_3_binds():
    for t, r in enumerate(R.oracle_run('births_fixed_3')):
        assert r['births'] == 3 * r['pairs'], (t, r['births'], r['pairs'])


def test_move_levy_binds():
    longest = max(r['longest_move'] for r in R.oracle_run('move_levy'))
    assert longest > 3, longest


def test_near_tie_census_leaves_clean_steps():
    """at least 3 clean steps in every regime and at least 120 of the 144 overall"""
    total, kinds = 0, dict(raster=0, hash=0, radius=0, death=0, low_edge=0)
    per_case = {}
    for name in R.NAMES:
        cen = [r['census'] for r in R.oracle_run(name)]
        clean = [t for t, c in enumerate(cen) if sum(c.values()) == 0]
        per_case[name] = len(clean)
        total += len(clean)
        for c in cen:
            for k, v in c.items():
                kinds[k] += v
        print('%-16s clean steps %s, soft %s' % (name, clean, [
            (t, {k: v for k, v in c.items() if v}) for t, c in enumerate(cen) if sum(c.values())]))
    print('clean steps: %d of %d; near-ties by kind: %s' % (total, 6 * len(R.NAMES), kinds))
    short = {n: k for n, k in per_case.items() if k < 3}
    assert not short, short
    assert total >= 120, total


def _births_of(st):
    lb = st.last_births
    return lb['child'], lb['parents'], lb['keys'], lb['start']


def _moved(st):
    dist = dict(zip(st.last_move['ids'].tolist(), st.last_move['dist'].tolist()))
    return lambda ids: np.array([dist.get(int(i), 0.0) for i in ids], np.float32)


def test_comparison_passes_the_oracle_against_itself():
    """the lockstep comparison of the GPU test, with a second oracle in the device's place:
    no difference in any step, position error 0, and the re-seating leaves the run as it was"""
    a, b = R.oracle_for('sexed_ages'), R.oracle_for('sexed_ages')
    for t in range(R.N_STEPS):
        ca, cb = R.S.step(a)[1:], R.S.step(b)[1:]
        da, ob = R.oracle_cols(a), R.oracle_cols(b)
        assert R.decision_differences(da, ob, ca, cb, _births_of(a), b.last_births) == []
        diffs, err = R.state_differences(da, ob, _moved(b))
        assert diffs == [] and err == 0.0, (t, diffs, err)
        if t % 2:
            R.reseat_positions(b, da)
        else:
            R.reseat(b, SimpleNamespace(step_index=a.step), da, a.max_id)


@pytest.mark.parametrize('name,wrong,step', [('max_age', dict(max_age=4), 0),
                                             ('repro_age', dict(repro_age=(2, 3)), 0),
                                             ('births_poisson', dict(n_births_lambda=1.8), 0)])
def test_comparison_catches_a_regime_one_off(name, wrong, step):
    """... and a side that runs the regime with one parameter one off differs in the named
    step, which is clean - nothing could excuse it"""
    a = R.oracle_for(name)
    b = R.oracle_for(name)
    for k, v in wrong.items():
        setattr(b.p, k, v)
    for t in range(step + 1):
        ca, cb = R.S.step(a)[1:], R.S.step(b)[1:]
    assert sum(R.census(b).values()) == 0
    diffs = R.decision_differences(R.oracle_cols(a), R.oracle_cols(b), ca, cb, _births_of(a),
                                   b.last_births)
    print(diffs)
    assert diffs, name


def test_state_comparison_catches_single_wrong_values():
    """one value of one column changed on one side: every column of (b) and (c) reports it"""
    a = R.oracle_for('default')
    R.S.step(a)
    ref = R.oracle_cols(a)
    dist = _moved(a)
    k = ref['ids'].size // 2
    for col, change in (('age', lambda v: v + 1), ('sex', lambda v: 1 - v),
                        ('z', lambda v: np.nextafter(v, np.float32(9))),
                        ('e', lambda v: np.nextafter(v, np.float32(9))),
                        ('fit', lambda v: v + 3 * np.spacing(v)),
                        ('x', lambda v: v + np.float32(1.5 * R.POS_TOL)),
                        ('geno', lambda v: v ^ np.uint64(1))):
        other = {c: v.copy() for c, v in ref.items()}
        if col in ('z', 'e'):
            other[col][-1, k] = change(other[col][-1, k])
        elif col == 'geno':
            other[col][k, 1, 1] = change(other[col][k, 1, 1])
        else:
            other[col][k] = change(other[col][k])
        diffs, _ = R.state_differences(other, ref, dist)
        assert len(diffs) == 1 and ('position' if col == 'x' else 'column ' + col) in diffs[0] \
            and 'id %d' % ref['ids'][k] in diffs[0], (col, diffs)


def test_witness_names_the_tie_or_none():
    """two sides that agree have no witness on a clean step; an individual that one side holds
    across a raster-cell boundary is named"""
    a = R.oracle_for('default')
    R.S.step(a)
    assert sum(R.census(a).values()) == 0
    ref = R.oracle_cols(a)
    mv = a.last_move
    post_move = (mv['ids'].copy(), mv['x'].copy(), mv['y'].copy())
    assert R.witness(a, ref, ref, post_move) is None
    assert R.witness(a, ref, ref, None) is None
    other = {c: v.copy() for c, v in ref.items()}
    k = int(np.argmax((ref['x'] > 1) & (ref['x'] < 23)))
    other['x'][k] = np.floor(ref['x'][k]) - np.float32(1e-5)
    w = R.witness(a, other, ref, None)
    assert w is not None and 'id %d ' % ref['ids'][k] in w and 'cell' in w, w
    moved = list(post_move)
    j = int(np.nonzero(mv['ids'] == ref['ids'][k])[0][0])
    moved[1] = moved[1].copy()
    moved[1][j] = other['x'][k]
    w = R.witness(a, ref, ref, tuple(moved))
    assert w is not None and 'after the movement' in w, w
