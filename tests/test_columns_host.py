"""The column checker of tests/_columns.py is sharp: it passes on a population the oracle's own
step produced and raises on each of six single-individual corruptions, two of them 2 f32 ulp
small.  This is what shows that tests/test_gpu_inherited_columns.py would fail on a kernel
that is subtly wrong.  No GPU."""
import numpy as np
import pytest

import gnx_oracle as O
import gnx_step as S
from _columns import check_columns

W = H = 40
N0 = 1500
L = 5000
F = np.float32


def _oracle_population():
    """10 oracle steps; then z with dominance and fit with deleterious loci, which State does
    not have, computed from the unpacked genomes (O.phenotype, O.fitness_deleterious: not the
    packed readers the checker uses)"""
    rng = np.random.RandomState(17)
    rasts = np.stack([np.ones((H, W)), np.tile(np.linspace(0, 1, W), (H, 1)),
                      np.tile(np.linspace(0, 1, H)[:, None], (1, W))]).astype(F)
    sel = rng.choice(np.setdiff1d(np.arange(L), [0, 63, 64, L - 1]), 40, replace=False)
    t_loci = [np.concatenate([[0, 63, 64, L - 1], sel[:8]]), sel[8:28], sel[28:34]]
    traits = [dict(loci=l, alpha=np.where(np.arange(l.size) % 2, -1.0, 1.0) / l.size,
                   layer=1 + t % 2, phi=0.05, gamma=1.0, univ_adv=False)
              for t, l in enumerate(t_loci)]
    paths = O.pack_bits(O.recomb_paths((rng.rand(64, L) < 2e-3).astype(np.uint8)
                                       * (np.arange(L) > 0)))
    st = S.State(rasts, S.Params(mating_radius=3.0, K_factor=1.0), 29, L=L, traits=traits,
                 paths_packed=paths)
    st.set_population(rng.rand(N0) * W, rng.rand(N0) * H, rng.randint(0, 4, N0), np.zeros(N0),
                      np.arange(N0))
    st.set_genomes(O.pack_genomes((rng.rand(N0, L, 2) < 0.5).astype(np.uint8)))
    for _ in range(10):
        S.step(st)
    assert st.N > 700 and (st.id >= N0).mean() > 0.5
    plain = dict(traits=traits, dom=None, delet_loci=np.zeros(0, np.int64),
                 delet_s=np.zeros(0))
    cols = dict(ids=st.id.copy(), x=st.x.copy(), y=st.y.copy(), e=st.e.T.copy(),
                z=st.z.T.copy(), fit=st.fit.copy(), geno=st.geno.copy())
    # the same population under dominance and with deleterious loci
    dom = np.zeros(L, np.uint8)
    for l in t_loci:
        dom[l[::2]] = 1
    arch = dict(traits=traits, dom=dom, delet_loci=sel[34:], delet_s=np.full(6, 0.002))
    G = O.unpack_genomes(st.geno, L)
    z = np.stack([O.phenotype(G, tr['loci'], tr['alpha'], dom) for tr in traits]).astype(F)
    w = O.fitness_traits(st.e.astype(np.float64), z.T.astype(np.float64),
                         [t['layer'] for t in traits], [t['phi'] for t in traits],
                         [t['gamma'] for t in traits], [t['univ_adv'] for t in traits])
    w = w * O.fitness_deleterious(G, arch['delet_loci'], arch['delet_s'])
    full = dict(cols, z=z, fit=w.astype(F))
    return rasts, plain, cols, arch, full


@pytest.fixture(scope='module')
def population():
    return _oracle_population()


def _copy(cols):
    return {k: v.copy() for k, v in cols.items()}


def _flip(geno, i, locus):
    geno[i, 0, locus >> 6] ^= np.uint64(1) << np.uint64(locus & 63)


def test_checker_passes_on_the_oracle_population(population):
    rasts, plain, cols, arch, full = population
    check_columns(cols, rasts, plain, True)           # State's own z, e and fit
    check_columns(full, rasts, arch, True)
    # slot order is free
    o = np.random.RandomState(1).permutation(full['ids'].size)
    check_columns({k: (v[:, o] if k in ('e', 'z') else v[o]) for k, v in full.items()},
                  rasts, arch, True)


CORRUPTIONS = ['z swapped', 'z 2 ulp', 'e of the neighbouring cell', 'fit 2 ulp',
               'trait bit flipped', 'deleterious bit flipped']


@pytest.mark.parametrize('what', CORRUPTIONS)
def test_checker_catches_a_single_corruption(population, what):
    rasts, _, _, arch, full = population
    c = _copy(full)
    i = 417 % c['ids'].size
    column = 'z of trait'
    if what == 'z swapped':
        j = int(np.nonzero(c['z'][1] != c['z'][1][i])[0][0])
        c['z'][:, [i, j]] = c['z'][:, [j, i]]
    elif what == 'z 2 ulp':
        v = c['z'][2, i]
        c['z'][2, i] = np.nextafter(np.nextafter(v, F(2)), F(2))
        assert 0 < c['z'][2, i] - v < 3e-7
    elif what == 'e of the neighbouring cell':
        cx, cy = int(c['x'][i]), int(c['y'][i])
        c['e'][1, i] = rasts[1, cy, cx + 1 if cx + 1 < W else cx - 1]
        assert c['e'][1, i] != rasts[1, cy, cx]
        column = 'e of layer 1'
    elif what == 'fit 2 ulp':
        v = c['fit'][i]
        c['fit'][i] = np.nextafter(np.nextafter(v, F(0)), F(0))
        column = 'fit is'
    elif what == 'trait bit flipped':
        _flip(c['geno'], i, int(arch['traits'][1]['loci'][3]))
    else:
        _flip(c['geno'], i, int(arch['delet_loci'][2]))
        column = 'fit is'
    with pytest.raises(AssertionError) as err:
        check_columns(c, rasts, arch, True)
    # the message names the individual and the column
    assert 'id %d:' % c['ids'][i if what != 'z swapped' else min(i, j, key=lambda k: c['ids'][k])] \
        in str(err.value), str(err.value)
    assert column in str(err.value), str(err.value)
    # ... and without the fitness check the genome still anchors z, the raster e
    if column != 'fit is':
        with pytest.raises(AssertionError):
            check_columns(c, rasts, arch, False)
    else:
        check_columns(c, rasts, arch, False)
