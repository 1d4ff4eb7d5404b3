"""The births enqueued before the held-back crossover (gnx_step_mid, xo_launch_late).

Handles above GNX_DD_MAX_CAP slots (600 000: bench.py's path) hold the deferred crossover of
step t back until step t + 1 has its pair list.  gnx_step_mid now reads the pair count, enqueues
the births, and only then hands that crossover to its stream, where it waits for the pair list
alone.  No kernel's inputs change, so everything must stay bit for bit what it was - and the
held-back crossover must be launched exactly once on every way out of the births: no pairs, too
many births for the handle, several handles stepped side by side, a walk's last step followed
by gnx_step.

The threshold is read once per process at gnx_create, so the late-path handles live in a child
process (tests/_births_first_worker.py, GNX_DD_MAX_CAP=1024, GNX_DD=0: 32 768 slots and fewer
take the path) that runs every scenario once and leaves one .npz; the twins under the default
threshold - the crossover launched as soon as its jobs are built - are made here.
Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _births_first_worker as W

pytestmark = pytest.mark.gpu

COLUMNS = ('ids', 'x', 'y', 'age', 'sex', 'fit', 'z', 'e', 'g')


@pytest.fixture(scope='module')
def late(tmp_path_factory):
    """the child's results: {'tag/column': array}"""
    out = str(tmp_path_factory.mktemp('births_first') / 'late.npz')
    env = dict(os.environ, GNX_DD_MAX_CAP='1024', GNX_DD='0')
    r = subprocess.run([sys.executable, os.path.join(W.HERE, '_births_first_worker.py'), out],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, 'worker exit code %d\n%s' % (r.returncode, r.stdout.decode()[-4000:])
    with np.load(out, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _pc(late, tag):
    return dict(zip((str(s) for s in late['pc_names']), (int(v) for v in late[tag + '/pc'])))


def _same(late, a, b):
    np.testing.assert_array_equal(late[a + '/hist'], late[b + '/hist'], err_msg='%s %s' % (a, b))
    for k in COLUMNS:
        np.testing.assert_array_equal(late['%s/%s' % (a, k)], late['%s/%s' % (b, k)],
                                      err_msg='%s %s: %s' % (a, b, k))


def test_the_route(late):
    """the walk took the path under test: the crossover from launch policy 2's site, lazy
    mortalities, the next movement launched ahead - and nothing flushed a crossover early"""
    pc = _pc(late, 'walk')
    assert pc['xo_launch_p2'] > 0 and pc['lazy_mortalities'] > 0 and pc['moves_ahead'] > 0, pc
    assert pc['lazy_mortalities'] == 8 + 4 and pc['moves_ahead'] == 8 + 4, pc
    # 15 steps: every one but the first finds the last step's crossover held back (the states'
    # download launches the last one: a flush, after the counters were read)
    assert pc['xo_launch_p2'] == 14 and pc['make_dense'] == 0, pc
    ps = _pc(late, 'steps')
    assert ps['xo_launch_p2'] == 14 and ps['lazy_mortalities'] == 0, ps
    assert late['walk/ids'].size > 5000


def test_walk_step_walk_equals_single_steps(late):
    """walk(9), gnx_step, walk(5) against 15 single steps of a twin on the same path: ids, x, y,
    age, sex, fitness, z, e and every living genome, id by id, and every step's counts"""
    _same(late, 'walk', 'steps')


def test_equals_the_twin_under_the_default_threshold(late, monkeypatch):
    """... and against 15 single steps of a twin created here, under the default threshold: its
    crossover goes on the side stream as soon as its jobs are built"""
    monkeypatch.setenv('GNX_DD', '0')
    dev, nat = W.make_main()
    hist = W.advance(dev, [('step', 15)])
    pc = dev.path_counts()
    assert pc['xo_launch_p2'] == 0 and pc['lazy_mortalities'] == 0, pc
    st = W.state(dev, nat)
    dev.close()
    np.testing.assert_array_equal(hist, late['walk/hist'])
    for k in COLUMNS:
        np.testing.assert_array_equal(st[k], late['walk/' + k], err_msg=k)


def test_a_step_without_pairs_behind_a_step_with_births(late):
    """(births, crossovers launched from policy 2's site, crossovers flushed) per step.  Step 3
    has b = 0: no pair, no birth, gnx_l_mate returns early - and the crossover of step 2's
    surviving offspring goes out there, once, from the policy's site.  The child has compared
    the genomes with the oracle's crossover replay right behind that step and at the end, and
    found no offspring left without its crossover (gnx_genome_info) after any step."""
    rec = late['nopairs/rec']
    assert rec.shape == (7, 3)
    assert (rec[[0, 1, 2, 4, 5, 6], 0] > 100).all() and rec[3, 0] == 0, rec
    assert tuple(rec[3, 1:]) == (1, 0), rec       # held back by step 2, launched in step 3
    assert tuple(rec[4, 1:]) == (0, 0), rec       # step 3 had nobody to cut
    assert (rec[[1, 2, 5, 6], 1] == 1).all() and (rec[:, 2] == 0).all(), rec


def test_births_that_do_not_fit(late):
    """the capacity code, the held-back crossover launched all the same (once, from the policy's
    site), and the living's genomes those of a twin before that step"""
    assert int(late['cap/rc'][0]) == 2, str(late['cap/err'])
    assert 'capacity exceeded' in str(late['cap/err'])
    assert tuple(late['cap/p2_flush']) == (1, 0)
    assert int(late['cap/deferred'][0]) == 0
    assert late['cap/a_ids'].size > 1000
    np.testing.assert_array_equal(late['cap/a_ids'], late['cap/b_ids'])
    np.testing.assert_array_equal(late['cap/a_g'], late['cap/b_g'])


@pytest.mark.parametrize('seed', [42, 7])
def test_two_handles_side_by_side(late, seed):
    """gnx_walk_many(4) and two gnx_step_many of two handles: each equals its own single-handle
    walk(4) and two steps"""
    _same(late, 'many%d' % seed, 'alone%d' % seed)
    pm, pa = _pc(late, 'many%d' % seed), _pc(late, 'alone%d' % seed)
    assert pm['xo_launch_p2'] == pa['xo_launch_p2'] == 5, (pm, pa)
    assert pm['moves_ahead'] == 0 and pa['moves_ahead'] == 3, (pm, pa)
