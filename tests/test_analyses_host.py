"""What the analysis calls of a Species share (geonomics_amd/structs/analyses.py) and what a new
analysis has to follow: which calls refuse a Species without (assigned) genomes and in which
words, how max_work is refused, and that structs/tiled.py refuses every analysis.  No GPU, no
library: the stand-in's handle has no calls, so a check that came after a device call would fail
with AttributeError.  The expected texts are written out here, not taken from the helpers."""
import types

import numpy as np
import pytest

from geonomics_amd.structs.analyses import SpeciesAnalyses

NO_GENOMES = 'the Species has no genomes (no gen_arch)'
UNASSIGNED = 'genomes are assigned at the end of the burn-in; burn the model in first'
# (who, method, positional arguments) of the calls that check both
CHECKED = [('run_gea', '_run_cca', ()), ('run_mmrr', '_run_mmrr', ()),
           ('run_mantel', '_run_mantel', ()),
           ('calc_spatial_structure', '_calc_spatial_structure', ()),
           ('calc_ld_decay', '_calc_ld_decay', ()), ('calc_ne', '_calc_ne', ()),
           ('calc_ancestry', '_calc_ancestry', (2,)), ('calc_roh', '_calc_roh', ()),
           ('calc_ibs_sharing', '_calc_ibs_sharing', ()), ('calc_ihs', '_calc_ihs', ()),
           ('calc_xpehh', '_calc_xpehh', (np.array([0, 0, 1, 1]),)),
           ('calc_ehh', '_calc_ehh', (0,))]
# (who, method, the unit of its max_work) of the calls that take a work limit
LIMITED = [('calc_spatial_structure', '_calc_spatial_structure', 'pair-words'),
           ('calc_ld_decay', '_calc_ld_decay', 'tile-words'),
           ('calc_ibs_sharing', '_calc_ibs_sharing', 'word steps'),
           ('calc_ihs', '_calc_ihs', 'word steps')]
# reach the device only through a method the tiled Species refuses (_group_counts)
THROUGH_A_REFUSED_ONE = {'_calc_fst', '_calc_diversity', '_calc_sfs'}


class _Reached(Exception):
    pass


class _Species(SpeciesAnalyses):
    """four individuals with L loci on a handle that has no calls at all"""

    def __init__(self, L=8, assigned=True):
        self._dev = types.SimpleNamespace(L=L, W64=16)
        self.gen_arch = None
        if L:
            rec = types.SimpleNamespace(_positions=np.arange(L),
                                        _rates=np.r_[0.0, np.full(L - 1, 0.01)])
            trt = types.SimpleNamespace(lyr_num=0, loci=np.array([1]))
            self.gen_arch = types.SimpleNamespace(traits={0: trt}, recombinations=rec)
        if assigned:
            self._genomes_assigned = True
        self._land_ref = types.SimpleNamespace(dim=(16, 16))

    def _geno_sample(self, individs):
        return np.arange(4, dtype=np.int64), np.arange(4, dtype=np.int64)


def _refusal(f, *args, **kw):
    with pytest.raises(ValueError) as err:
        f(*args, **kw)
    return str(err.value)


def test_the_mixin_keeps_no_state_and_no_attribute_hooks():
    for name in ('__init__', '__getattr__', '__setattr__', '__getattribute__', '__slots__'):
        assert name not in vars(SpeciesAnalyses), name
    assert SpeciesAnalyses.__bases__ == (object,)


@pytest.mark.parametrize('who,method,args', CHECKED, ids=[c[0] for c in CHECKED])
def test_a_call_refuses_a_species_without_assigned_genomes(who, method, args):
    assert _refusal(getattr(_Species(L=0), method), *args) == '%s: %s' % (who, NO_GENOMES)
    assert _refusal(getattr(_Species(assigned=False), method), *args) == \
        '%s: %s' % (who, UNASSIGNED)


def test_the_counting_calls_refuse_bare_and_do_not_ask_for_the_burn_in():
    assert _refusal(_Species(L=0)._group_counts, None) == NO_GENOMES
    assert _refusal(_Species(L=0)._calc_diversity_map) == NO_GENOMES
    # genomes that are not assigned yet: both go on to their next step
    spp = _Species(assigned=False)
    spp._geno_sample = lambda individs: (_ for _ in ()).throw(_Reached())
    with pytest.raises(_Reached):
        spp._group_counts(None)
    assert _refusal(spp._calc_diversity_map, win=2).startswith('win: an odd number')


@pytest.mark.parametrize('who,method,what', LIMITED, ids=[c[0] for c in LIMITED])
def test_max_work_is_a_positive_integer_in_the_calls_unit(who, method, what):
    for bad in (0, True, 1.5):
        assert _refusal(getattr(_Species(), method), max_work=bad) == \
            '%s: max_work: a positive number of %s (got %r)' % (who, what, bad)


def test_the_tiled_species_refuses_every_analysis():
    from geonomics_amd.structs.species import Species
    from geonomics_amd.structs.tiled import _NOT_TILED, TiledSpecies
    for name in _NOT_TILED:
        assert callable(getattr(Species, name)), name
        for args, kw in (((), {}), ((1, 2), dict(predictors=('geo', 'cost')))):
            with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
                getattr(TiledSpecies, name)(object(), *args, **kw)
    analyses = {n for n, f in vars(SpeciesAnalyses).items() if callable(f) and
                (n.startswith(('_calc_', '_run_')) or
                 n in ('_get_lineage_dicts', '_check_coalescence'))}
    assert analyses - set(_NOT_TILED) == THROUGH_A_REFUSED_ONE
