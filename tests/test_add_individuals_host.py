"""Model.add_individuals, the part that needs no device: the argument rules of an introduction
(reference structs/species.py:1645-1840, sim/model.py:3228-3335) as the pure functions
structs/species.py keeps them in, and the public signature."""
import inspect
import types

import numpy as np
import pytest

from geonomics_amd.structs import species as S

DIM = (40, 30)            # land dims are [x, y]
SRC = [17, 3, 8, 25, 11, 4]


def plan(n=None, coords=(1.0, 2.0), individs=None, source_ids=SRC, dim=DIM):
    return S._introduction_plan(n, coords, individs, source_ids, dim)


# ------------------------------------------------------------------ who is taken, in which order
def test_n_takes_the_smallest_ids_in_ascending_order():
    ids, xy = plan(n=4)
    np.testing.assert_array_equal(ids, [3, 4, 8, 11])
    assert ids.dtype == np.int64 and xy.dtype == np.float32 and xy.shape == (4, 2)


def test_individs_are_taken_in_ascending_id_order_and_coords_follow_that_order():
    coords = [[1, 1], [2, 2], [3, 3]]
    ids, xy = plan(individs=[25, 3, 11], coords=coords)
    np.testing.assert_array_equal(ids, [3, 11, 25])
    # the i-th of the chosen (ascending) gets coords[i], whatever order individs came in
    np.testing.assert_array_equal(xy, np.float32(coords))


def test_n_zero_and_the_whole_source():
    ids, xy = plan(n=0)
    assert ids.size == 0 and xy.shape == (0, 2)
    ids, _ = plan(n=len(SRC))
    np.testing.assert_array_equal(ids, sorted(SRC))


# ------------------------------------------------------------------ exactly one of n / individs
def test_both_n_and_individs_is_refused():
    with pytest.raises(AssertionError, match="exactly one of 'n' and 'individs'"):
        plan(n=2, individs=[3, 4])


def test_neither_n_nor_individs_is_refused():
    with pytest.raises(AssertionError, match="exactly one of 'n' and 'individs'"):
        plan()


def test_n_larger_than_the_source_is_refused():
    with pytest.raises(AssertionError, match='must not exceed the size of the source'):
        plan(n=len(SRC) + 1)


@pytest.mark.parametrize('n', [-1, 2.0, True, 'three'])
def test_n_must_be_a_non_negative_int(n):
    with pytest.raises(AssertionError, match='non-negative int'):
        plan(n=n)


def test_individs_not_in_the_source_are_refused():
    with pytest.raises(AssertionError, match='do not exist in the source'):
        plan(individs=[3, 5], coords=(1, 1))


def test_individs_listed_twice_are_refused():
    with pytest.raises(AssertionError, match='more than once'):
        plan(individs=[3, 3], coords=(1, 1))


# ------------------------------------------------------------------ coords
def test_one_pair_is_broadcast_to_everybody():
    for c in ((5.5, 6.25), [[5.5, 6.25]], np.array([5.5, 6.25])):
        _, xy = plan(n=3, coords=c)
        np.testing.assert_array_equal(xy, np.float32([[5.5, 6.25]] * 3))


def test_one_pair_for_one_individual():
    _, xy = plan(n=1, coords=[[7, 8]])
    np.testing.assert_array_equal(xy, np.float32([[7, 8]]))


@pytest.mark.parametrize('coords', [[[1, 1], [2, 2]], [1, 2, 3], [[1, 2, 3]] * 3, 5.0])
def test_coords_of_another_shape_are_refused(coords):
    with pytest.raises(AssertionError, match="'coords' must be a single x,y pair"):
        plan(n=3, coords=coords)


def test_the_border_is_dim_minus_0_001_inclusive():
    _, xy = plan(n=2, coords=[[DIM[0] - 0.001, 0.0], [0.0, DIM[1] - 0.001]])
    # what the library is handed still lies on the landscape
    assert (xy[:, 0] < DIM[0]).all() and (xy[:, 1] < DIM[1]).all() and (xy >= 0).all()


@pytest.mark.parametrize('c', [(DIM[0] - 0.0009, 1.0), (1.0, DIM[1] - 0.0009), (-1e-6, 1.0),
                               (1.0, -1e-6), (DIM[0], 1.0), (35.0, 35.0), (np.nan, 1.0)])
def test_coords_off_the_landscape_are_refused(c):
    # (35, 35): x within dim[0] = 40 but y beyond dim[1] = 30 - the dims are [x, y]
    with pytest.raises(AssertionError, match="must lie on the recipient Species' Landscape"):
        plan(n=2, coords=c)
    with pytest.raises(AssertionError, match="must lie on the recipient Species' Landscape"):
        plan(n=2, coords=[(1.0, 1.0), c])


# ------------------------------------------------------------------ compatibility of the two Species
def _trait(**kw):
    d = dict(name='trait_0', phi=0.05, lyr_num=1, max_alpha_mag=None, gamma=1, univ_adv=False,
             n_loci=4)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _spp(traits='default', **kw):
    rec = dict(_rates=np.array([0.5, 0.01, 0.01]), _r_distr_alpha=None, _r_distr_beta=None,
               _jitter_breakpoints=False)
    ga = dict(L=64, sex=False, use_tskit=False, x=2)
    top = dict(K_layer=0, selection=True, sex_ratio=0.5, move=True)
    for k, v in kw.items():
        (rec if k in rec else ga if k in ga else top)[k] = v
    if traits == 'default':
        traits = {0: _trait(), 1: _trait(name='trait_1', lyr_num=0, univ_adv=True, gamma=2)}
    gen_arch = types.SimpleNamespace(recombinations=types.SimpleNamespace(**rec), traits=traits,
                                     **ga)
    return types.SimpleNamespace(gen_arch=gen_arch, **top)


def test_equal_species_pass_and_free_attributes_may_differ():
    S._check_introduction_compat(_spp(), _spp())
    # the number of loci of a Trait may differ (independent mutation), as in the reference
    b = _spp(traits={0: _trait(n_loci=9), 1: _trait(name='trait_1', lyr_num=0, univ_adv=True,
                                                  gamma=2)})
    S._check_introduction_compat(_spp(), b)
    S._check_introduction_compat(_spp(traits=None), _spp(traits=None))


@pytest.mark.parametrize('attr,val', [('K_layer', 1), ('selection', False), ('sex_ratio', 0.4),
                                      ('move', False)])
def test_species_attributes_must_agree(attr, val):
    with pytest.raises(AssertionError, match="must have the same '%s'" % attr):
        S._check_introduction_compat(_spp(), _spp(**{attr: val}))


def test_genome_length_must_agree():
    with pytest.raises(AssertionError, match="as long as the recipient's"):
        S._check_introduction_compat(_spp(), _spp(L=128))


@pytest.mark.parametrize('attr,val', [('sex', True), ('use_tskit', True), ('x', 1)])
def test_gen_arch_attributes_must_agree(attr, val):
    with pytest.raises(AssertionError, match="GenomicArchitectures .* the same '%s'" % attr):
        S._check_introduction_compat(_spp(), _spp(**{attr: val}))


@pytest.mark.parametrize('attr,val', [('_rates', np.array([0.5, 0.02, 0.01])),
                                      ('_rates', np.array([0.5, 0.01])),
                                      ('_r_distr_alpha', 0.5), ('_r_distr_beta', 2.0),
                                      ('_jitter_breakpoints', True)])
def test_recombination_attributes_must_agree(attr, val):
    with pytest.raises(AssertionError, match="Recombinations .* same '%s'" % attr):
        S._check_introduction_compat(_spp(), _spp(**{attr: val}))


def test_traits_must_match_in_number_and_presence():
    with pytest.raises(AssertionError, match='cannot be added to a Species without them'):
        S._check_introduction_compat(_spp(traits=None), _spp())
    with pytest.raises(AssertionError, match='as many Traits'):
        S._check_introduction_compat(_spp(), _spp(traits={0: _trait()}))
    with pytest.raises(AssertionError, match='as many Traits'):
        S._check_introduction_compat(_spp(), _spp(traits=None))


@pytest.mark.parametrize('attr,val', [('name', 'other'), ('phi', 0.1), ('lyr_num', 0),
                                      ('max_alpha_mag', 0.3), ('gamma', 2), ('univ_adv', True)])
def test_trait_attributes_must_agree(attr, val):
    # (the loop the reference means to run: every listed attribute of every Trait)
    b = _spp(traits={0: _trait(**{attr: val}),
                     1: _trait(name='trait_1', lyr_num=0, univ_adv=True, gamma=2)})
    with pytest.raises(AssertionError, match="'%s' of Trait 0 must be the same" % attr):
        S._check_introduction_compat(_spp(), b)


def test_a_phi_raster_is_compared_element_by_element():
    phi = np.full((3, 4), 0.05)
    a = _spp(traits={0: _trait(phi=phi)})
    S._check_introduction_compat(a, _spp(traits={0: _trait(phi=phi.copy())}))
    other = phi.copy()
    other[1, 2] = 0.06
    with pytest.raises(AssertionError, match="'phi' of Trait 0"):
        S._check_introduction_compat(a, _spp(traits={0: _trait(phi=other)}))


# ------------------------------------------------------------------ the public signature
def test_model_add_individuals_has_the_reference_signature():
    from geonomics_amd.sim.model import Model
    sig = inspect.signature(Model.add_individuals)
    assert list(sig.parameters) == ['self', 'n', 'coords', 'recip_spp', 'source_spp',
                                    'source_msprime_params', 'individs']
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d['n'] is inspect.Parameter.empty and d['coords'] is inspect.Parameter.empty
    assert d['recip_spp'] == 0 and d['source_spp'] is None
    assert d['source_msprime_params'] is None and d['individs'] is None


def test_species_add_individuals_takes_the_reference_arguments():
    sig = inspect.signature(S.Species._add_individuals)
    assert list(sig.parameters)[:7] == ['self', 'n', 'coords', 'land', 'source_spp',
                                        'source_msprime_params', 'individs']


def test_a_tiled_species_refuses():
    from geonomics_amd.structs.tiled import TiledSpecies
    with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
        TiledSpecies._add_individuals(object(), 3, (1, 1))


def test_the_binding_exports_the_transplant():
    from geonomics_amd import _native as nat
    assert 'gnx_transplant' in nat.EXPORTS and callable(nat.Device.transplant)
    assert nat.GnxError('x').code is None
