"""Model.run_gea on the device (csrc/gnx_gea.hip, sim/gea.py, Species._run_cca): the
cross-products against numpy / torch-fp64 on the downloaded genotypes and columns, and the whole
analysis against the host path (tests/test_gea_host.py, which ties that path to the
reference's own _run_cca and to sklearn) on the same downloaded inputs.  Needs an MI355X.

Bounds.  C = D^T D and s = D^T 1 are integers: bit-equal.  D^T Z, Z^T Z, Z^T 1 are fp64 sums of
N terms (d z is exact: d in {0, 1, 2}); any order of summation stays within
N 2^-53 sum|d||z| of any other, which is the bound asserted against numpy.  loci_df and var_df
come from those: 1e-9 of the largest |entry|, the host test's bar.  ind_df is one fp32 product
D M with M = R / (2 sd): n_loci 2^-23 (|D| |M|) per entry, the product bound of DESIGN.md 9."""
import warnings

import numpy as np
import pytest

from test_gpu_parity import native
from test_gpu_product_path import _make, _paths, L as PP_L
from test_gea_host import GOLDEN, BAR, OUTPUTS

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
EPS32 = 2.0 ** -23


def _dosages_at(packed, loci):
    """dosages float64 [n][len(loci)] on the GPU of packed genomes uint64 [n][2][W64]"""
    import torch
    loci = torch.as_tensor(np.asarray(loci, np.int64), device='cuda')
    word, bit = loci >> 6, loci & 63
    out = []
    for r0 in range(0, packed.shape[0], 2048):
        t = torch.from_numpy(np.ascontiguousarray(packed[r0:r0 + 2048]).view(np.int64)).cuda()
        b = (t[:, :, word] >> bit) & 1
        out.append((b[:, 0] + b[:, 1]).to(torch.float64))
    return torch.cat(out)


def _int_gram(D):
    import torch
    return ((D.T @ D).round().to(torch.int64).cpu().numpy(),
            D.sum(dim=0).round().to(torch.int64).cpu().numpy())


def _columns(dev, nat, lyr, slots=None):
    """Z = [e[:, lyr], x, y] float64 [n][3] as the device holds them"""
    Z = np.column_stack([dev.download(nat.F_E)[lyr], dev.download(nat.F_X),
                         dev.download(nat.F_Y)]).astype(np.float64)
    return Z if slots is None else Z[slots]


@pytest.fixture(scope='module')
def fixture_dev():
    """the population of tests/golden/g18_gea.npz on a handle: N = 400 (not a multiple of 64),
    L = 96, on the fixture's 24 x 24 landscape (layer 1: the west-east gradient)"""
    import gnx_oracle as O
    nat = native()
    f = np.load(GOLDEN)
    D = f['dosages'].astype(np.int64)
    n, L = D.shape
    dev = nat.Device(24, 24, 2, L=L, cap_inds=n + 64, cap_rows=n + 64, seed=18)
    dev.upload_rasters(np.stack([np.ones((24, 24)),
                                 np.tile(np.linspace(0, 1, 24), (24, 1))]).astype(np.float32))
    dev.set_species_params(nat.default_species_params())
    top = np.nextafter(np.float32(24), np.float32(0))
    dev.upload_population(np.minimum(f['x'].astype(np.float32), top),
                          np.minimum(f['y'].astype(np.float32), top), np.zeros(n), np.zeros(n),
                          f['ids'])
    dev.upload_genomes(O.pack_genomes(np.stack([D >= 1, D == 2], axis=2).astype(np.uint8)))
    yield dev, nat, D
    dev.close()


CASES = ['all', 'loci', 'slots', 'both']


def _case(case, n, L, seed=0):
    rng = np.random.RandomState(seed)
    loci = np.arange(L)
    slots = None
    if case in ('loci', 'both'):
        loci = np.sort(rng.choice(L, L // 3, replace=False))
        loci[-1] = L - 1
    if case in ('slots', 'both'):
        slots = rng.choice(n, 131, replace=False).astype(np.int64)      # 2 words + 3 individuals
    return loci, slots


@pytest.mark.parametrize('case', CASES)
def test_locus_gram_exact_on_the_fixture(fixture_dev, case):
    dev, nat, D = fixture_dev
    loci, slots = _case(case, *D.shape)
    Dn = D[:, loci] if slots is None else D[slots][:, loci]
    C, s = dev.geno_locus_gram(loci, slots)
    np.testing.assert_array_equal(C, Dn.T @ Dn)
    np.testing.assert_array_equal(s, Dn.sum(axis=0))
    C2, s2 = dev.geno_locus_gram(loci, slots)                # back to back: the same
    np.testing.assert_array_equal(C2, C)
    np.testing.assert_array_equal(s2, s)


@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_locus_gram_padding_bits_never_count(fixture_dev, n):
    dev, nat, D = fixture_dev
    slots = np.arange(n, dtype=np.int64) * 3
    C, s = dev.geno_locus_gram(np.arange(D.shape[1]), slots)
    np.testing.assert_array_equal(C, D[slots].T @ D[slots])
    np.testing.assert_array_equal(s, D[slots].sum(axis=0))


@pytest.mark.parametrize('case', CASES)
def test_locus_cross_within_the_fp64_summation_bound(fixture_dev, case):
    dev, nat, D = fixture_dev
    loci, slots = _case(case, *D.shape, seed=1)
    Dn = (D[:, loci] if slots is None else D[slots][:, loci]).astype(np.float64)
    Z = _columns(dev, nat, 1, slots)
    n = Dn.shape[0]
    DtZ, ZtZ, Zt1 = dev.geno_locus_cross(loci, 1, slots)
    worst = 0.0
    for got, ref, bound in ((DtZ, Dn.T @ Z, n * U53 * (Dn.T @ np.abs(Z))),
                            (ZtZ, Z.T @ Z, n * U53 * (np.abs(Z).T @ np.abs(Z))),
                            (Zt1, Z.sum(axis=0), n * U53 * np.abs(Z).sum(axis=0))):
        err = np.abs(got - ref)
        worst = max(worst, (err / np.maximum(bound, 1e-300)).max())
        assert (err <= bound).all()
    print('%s: worst error / bound %.3g' % (case, worst))
    again = dev.geno_locus_cross(loci, 1, slots)              # fixed order: bit-equal
    for a, b in zip(again, (DtZ, ZtZ, Zt1)):
        np.testing.assert_array_equal(a, b)
    # layer 0 is constant 1: env's column of D^T Z is D^T 1
    DtZ0, ZtZ0, Zt10 = dev.geno_locus_cross(loci, 0, slots)
    np.testing.assert_array_equal(DtZ0[:, 0], Dn.sum(axis=0))
    assert ZtZ0[0, 0] == n and Zt10[0] == n


def test_fixture_analysis_from_device_products(fixture_dev):
    """the host recurrence fed by the device's products, against the same fed by numpy's on
    the downloaded columns"""
    from geonomics_amd.sim import gea as G
    dev, nat, D = fixture_dev
    loci = np.arange(D.shape[1])
    C, s = dev.geno_locus_gram(loci)
    DtZ, ZtZ, Zt1 = dev.geno_locus_cross(loci, 1)
    Df = D.astype(np.float64)
    got = G.cca_from_cross_products(C, s, DtZ, ZtZ, Zt1, D.shape[0], lambda M: Df @ M)
    ref = G.cca_from_cross_products(*G.numpy_cross_products(D, _columns(dev, nat, 1)),
                                    D.shape[0], lambda M: Df @ M)
    for k in OUTPUTS:
        err = np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max()
        print('%s: %.3g (smallest kept eigenvalue ratio %.3g)' % (k, err, got['min_kept_ratio']))
        assert err <= BAR, (k, err, got['min_kept_ratio'])


def test_limits(fixture_dev):
    dev, nat, D = fixture_dev
    L = D.shape[1]
    for call in (lambda l, **kw: dev.geno_locus_gram(l, **kw),
                 lambda l, **kw: dev.geno_locus_cross(l, 1, **kw)):
        with pytest.raises(nat.GnxError, match='8192'):
            call(np.zeros(0, np.int32))
        with pytest.raises(nat.GnxError, match='8192'):
            call(np.arange(8193))
        for bad in ([3, 3], [5, 4], [0, L], [-1, 2]):
            with pytest.raises(nat.GnxError, match='ascending, distinct'):
                call(bad)
        with pytest.raises(nat.GnxError, match='slot out of range'):
            call([0, 1], slots=np.array([0, dev.N]))
    with pytest.raises(nat.GnxError, match='layer'):
        dev.geno_locus_cross([0, 1], 2)
    empty = nat.Device(16, 16, 1, L=1000, cap_inds=256, cap_rows=256, seed=1)
    empty.upload_rasters(np.ones((1, 16, 16), np.float32))
    empty.set_species_params(nat.default_species_params())
    empty.upload_population(np.ones(10), np.ones(10), np.zeros(10), np.zeros(10), np.arange(10))
    with pytest.raises(nat.GnxError, match='genomes not assigned'):
        empty.geno_locus_gram([0, 1])
    with pytest.raises(nat.GnxError, match='genomes not assigned'):
        empty.geno_locus_cross([0, 1], 0)
    empty.close()


def test_products_on_a_walked_population_with_a_pending_crossover():
    """the product path (2^20 slots: lazy mortality, the crossover launched behind the next
    step, blocks shared with parents): after a dozen steps, with this step's offspring still
    waiting for their genomes, both calls cut the crossover and read everybody alive"""
    nat = native()
    dev, _ = _make(_paths(False), cap_inds=1 << 20, cap_rows=1 << 15, N=12000, K_factor=8.0)
    for T in (4, 3, 5):
        dev.walk(T, False, True)
    hist = dev.walk_history()
    assert hist[2].sum() > 0                                   # some have died
    pc = dev.path_counts()
    assert pc['lazy_mortalities'] > 0 and pc['xo_launch_p2'] > 0, pc
    rng = np.random.RandomState(12)
    loci = np.sort(rng.choice(PP_L, 2500, replace=False))
    loci[0], loci[-1] = 0, PP_L - 1                            # the first word and the last
    dev.age()
    dev.move()
    dev.pop_dynamics_mate(False)
    assert dev.counts()[1] > 0 and dev.genome_info()['deferred'] == 1
    n = dev.N
    C, s = dev.geno_locus_gram(loci)                           # everybody, newborns included
    assert dev.genome_info()['deferred'] == 0
    D = _dosages_at(dev.download_genomes(np.arange(n)), loci)
    assert D.shape == (n, loci.size)
    C_ref, s_ref = _int_gram(D)
    np.testing.assert_array_equal(C, C_ref)
    np.testing.assert_array_equal(s, s_ref)
    slots = rng.choice(n, 5000, replace=False).astype(np.int64)
    import torch
    Ds = D[torch.as_tensor(slots, device='cuda')]
    C, s = dev.geno_locus_gram(loci, slots)
    C_ref, s_ref = _int_gram(Ds)
    np.testing.assert_array_equal(C, C_ref)
    np.testing.assert_array_equal(s, s_ref)
    Z = torch.as_tensor(_columns(dev, nat, 1), device='cuda')
    DtZ, ZtZ, Zt1 = dev.geno_locus_cross(loci, 1)
    err = np.abs(DtZ - (D.T @ Z).cpu().numpy())
    bound = n * U53 * (D.T @ Z.abs()).cpu().numpy()
    print('walked: D^T Z worst error / bound %.3g' % (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all()
    Zn = Z.cpu().numpy()
    assert (np.abs(ZtZ - Zn.T @ Zn) <= n * U53 * (np.abs(Zn).T @ np.abs(Zn))).all()
    assert (np.abs(Zt1 - Zn.sum(axis=0)) <= n * U53 * np.abs(Zn).sum(axis=0)).all()
    dev.close()


# ------------------------------------------------------------------ the public call
def _small_model(seed):
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    mod = gnx.make_model(small_params(seed=seed))
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(12, 'main', verbose=False)
    return mod


def test_model_run_gea_matches_the_host_path():
    from geonomics_amd.sim import gea as G
    mod = _small_model(5)
    spp = mod.comm[0]
    ids = np.array([*spp])
    with pytest.warns(UserWarning, match='does not plot'):
        res = mod.run_gea()                                     # the default call
    assert sorted(res) == ['ids', 'ind_df', 'loci_df', 'trait_loci', 'var_df']
    np.testing.assert_array_equal(res['ids'], ids)
    assert (np.diff(res['ids']) > 0).all()
    trt = spp.gen_arch.traits[0]
    np.testing.assert_array_equal(res['trait_loci'], trt.loci)
    # the same inputs, downloaded: mean genotypes and columns in ascending-id order
    D = np.rint(mod.get_genotypes() * 2).astype(np.int64)
    n, L = D.shape
    assert n > L + 3
    Z = np.column_stack([mod.get_e(lyr_num=trt.lyr_num), mod.get_x(), mod.get_y()])
    Df = D.astype(np.float64)
    ref = G.cca_from_cross_products(*G.numpy_cross_products(D, Z), n, lambda M: Df @ M)
    for k in ('loci_df', 'var_df'):
        err = np.abs(res[k] - ref[k]).max() / np.abs(ref[k]).max()
        print('%s: %.3g of the largest entry (smallest kept eigenvalue ratio %.3g)'
              % (k, err, ref['min_kept_ratio']))
        assert err <= BAR, (k, err, ref['min_kept_ratio'])
    # the scores: M = R / (2 sd), recovered from the host path by feeding it the identity
    M = {}
    G.cca_from_cross_products(*G.numpy_cross_products(D, Z), n,
                              lambda m: (M.setdefault('M', m), Df @ m)[1])
    bound = L * EPS32 * (Df @ np.abs(M['M']))
    err = np.abs(res['ind_df'] - ref['ind_df'])
    print('ind_df: worst error / bound %.3g' % (err / bound).max())
    assert (err <= bound).all()
    # the extensions, and the table on request
    some = ids[::2][::-1]
    loci = np.arange(8, 40)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        sub = mod.run_gea(plot=False, individs=some, loci=loci, gea_df=True)
    np.testing.assert_array_equal(sub['ids'], ids[::2])
    Ds = D[::2][:, loci]
    Dsf = Ds.astype(np.float64)
    ref = G.cca_from_cross_products(*G.numpy_cross_products(Ds, Z[::2]), Ds.shape[0],
                                    lambda M: Dsf @ M)
    for k in ('loci_df', 'var_df'):
        assert np.abs(sub[k] - ref[k]).max() <= BAR * np.abs(ref[k]).max(), k
    np.testing.assert_array_equal(sub['gea_df'], np.column_stack([Ds / 2.0, Z[::2]]))
    with pytest.raises(ValueError, match='Valid methods'):
        mod.run_gea(method='rda')
    with pytest.raises(ValueError, match='no Trait'):
        mod.run_gea(trt=9, plot=False)
    with pytest.raises(ValueError, match='not alive'):
        mod.run_gea(plot=False, individs=[ids[-1] + 1000])
    from geonomics_amd.structs.tiled import TiledSpecies
    with pytest.raises(NotImplementedError):
        TiledSpecies._run_cca(spp)


def test_run_gea_leaves_the_model_as_it_was():
    """get_genotypes, get_x and the next walk step: byte-identical with and without a run_gea
    call in between"""
    a, b = _small_model(7), _small_model(7)
    a.run_gea(plot=False)
    for step in range(2):
        np.testing.assert_array_equal(np.array([*a.comm[0]]), np.array([*b.comm[0]]))
        assert a.get_genotypes(biallelic=True).tobytes() == b.get_genotypes(biallelic=True).tobytes()
        assert a.get_x().tobytes() == b.get_x().tobytes()
        assert a.get_e().tobytes() == b.get_e().tobytes()
        a.walk(1, 'main', verbose=False)
        b.walk(1, 'main', verbose=False)
        if step == 0:
            a.run_gea(plot=False, loci=np.arange(20))
