"""k_pair_compact with the loads of its four rounds issued together.

A workgroup of 256 threads takes 1024 slots, a thread four of them; every load of the kernel now
goes out level by level for all four rounds, from indices clamped into the live range (items past
N repeat item N - 1, an item without a mate stands in for its mate).  What can go wrong is the
tail and the stand-ins: so N sits around one workgroup's four rounds and one past a block boundary
(1, 255, 256, 257, 1 023, 1 024, 1 025, 4 097), nobody is kept (every flag 0, most mates -1),
everybody is kept, and everybody sits in one hash cell (mates anywhere in the block, and beyond).

The pair list - (focal, mate) in slot order, and its count - is compared with the oracle's
find_pairs (oracle/gnx_step.py) and with the same library given the keep mask instead of drawing
it (gnx_op_find_pairs(keep): the C-ABI has no entry that takes the mate array itself).  The
midpoints are not readable through the C-ABI either; their density raster is (GNX_R_NPAIRS), and
it is compared with the library's own density of the midpoints computed here, in float32, from
the device's positions and pair list: both are splines through counts of the same points on the
same lattice - integers - evaluated in float64, so they agree to rounding (1e-9 of the largest
value asked; a midpoint in another bin moves a count by one, i.e. the raster by about
1 / (window area) somewhere).  The device-driven path (GNX_DD=2: the same kernel under a
capacity-sized grid, counts on the device) has no read-out of its own: a walk through it against
single host-driven steps, everybody by id.  Needs an MI355X."""
import numpy as np
import pytest

import gnx_draws as D
import gnx_step as S
from test_gpu_parity import make_dev, upload_simple, native
from test_gpu_compaction_rounds import _clumps, _model, _walk_against_steps, R

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 1023, 1024, 1025, 4097]
CASES = {'nobody': 0.0, 'everybody': 1.0, 'one_cell': 0.5}


def _layout(case, n, rng):
    if case == 'one_cell':
        # everybody within 0.1 of one point well inside a hash cell (cells are R / 2 or wider)
        W = 16
        ids = np.sort(rng.choice(10 ** 6, n, replace=False)) + 1000
        x = (8.3 + rng.rand(n) * 0.1).astype(np.float32)
        y = (8.3 + rng.rand(n) * 0.1).astype(np.float32)
        return x, y, ids, W
    x, y, ids, _, W = _clumps(rng, n)
    return x, y, ids, W


def oracle_pairs(x, y, ids, sex, W, seed, step, b, sexed):
    """gnx_step.find_pairs on the population in the device's slot order -> (focal id, mate id)
    rows in pair-list order, and the oracle's state"""
    st = S.State(np.ones((1, W, W), np.float32),
                 S.Params(mating_radius=R, b=b, sexed=bool(sexed)), seed)
    st.set_population(x, y, np.zeros(len(x), np.int32), sex, ids)
    st.step = step
    S.sort_by_cell(st)
    pr = S.find_pairs(st)
    return st.id[pr].reshape(-1, 2), st


@pytest.mark.parametrize('sexed', [0, 1])
@pytest.mark.parametrize('case', sorted(CASES))
@pytest.mark.parametrize('n', SIZES)
def test_pair_list_midpoints_and_count(n, case, sexed):
    nat = native()
    rng = np.random.RandomState(7000 + n)
    seed, step, b = 4242, 6, CASES[case]
    x, y, ids, W = _layout(case, n, rng)
    sex = rng.randint(0, 2, n).astype(np.uint8) if sexed else np.zeros(n, np.uint8)
    exp, st = oracle_pairs(x, y, ids, sex, W, seed, step, b, sexed)
    dev = make_dev(W, W, cap=(2 * n + 9) | 1, seed=seed, mating_radius=R, b=b, sexed=sexed)
    upload_simple(dev, x, y, ids=ids, sex=sex)
    dev.step_index = step
    mate, pairs = dev.op_find_pairs()
    id_s = dev.download(nat.F_ID)
    np.testing.assert_array_equal(id_s, st.id)                  # the same slot order
    np.testing.assert_array_equal(id_s[pairs].reshape(-1, 2), exp)     # list, order and count
    if case == 'nobody':
        assert len(pairs) == 0 and (mate == -1).all()
    elif n >= 255:
        # (the case is not an empty one.  Fewest where b = 0.5 meets the sex filter: a kept female
        # whose mate is male, n / 8 expected - half of that)
        assert len(pairs) > n // 16
    # the same library, the keep mask injected (by slot)
    keep = D.keep_draws(seed, id_s, step, b)
    mate2, pairs2 = dev.op_find_pairs(keep)
    np.testing.assert_array_equal(pairs2, pairs)
    # the midpoints k_pair_compact wrote, through their density
    if len(pairs):
        xs, ys = dev.download(nat.F_X), dev.download(nat.F_Y)
        mx = (xs[pairs[:, 0]] + xs[pairs[:, 1]]) / np.float32(2.0)
        my = (ys[pairs[:, 0]] + ys[pairs[:, 1]]) / np.float32(2.0)
        dev.pop_dynamics(True, False)
        assert dev.counts()[1] == len(pairs)                    # one birth per pair
        got = dev.download_raster(nat.R_NPAIRS)
        _, ref = dev.op_density(mx, my)
        assert ref.max() > 0
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9 * ref.max())
    dev.close()


@pytest.mark.parametrize('n', SIZES)
def test_device_driven_path(n, monkeypatch):
    """GNX_DD=2: walk(4) - three device-driven steps and the walk's host-driven last - against four
    single steps of a twin: the counts of every step and everybody by id, genomes included (the
    offspring's ids and parents follow the pair list's order)"""
    monkeypatch.setenv('GNX_DD', '2')
    cap = (2 * n + 64) | 3
    a, nat = _model(n, cap)
    b, _ = _model(n, cap)
    hist = _walk_against_steps(a, b, nat, 4)
    if n >= 255:
        assert sum(h[1] for h in hist) > 0, hist
        assert a.totals()['dd_steps'] == 3 and b.totals()['dd_steps'] == 0
    a.close()
    b.close()
