"""Weighted relationship matrices on the device (csrc/gnx_grm.hip: f32 MFMA, fp64 sums) through
the C-ABI and through the Model (calc_grm, calc_heritability, predict_breeding_values), against
gnx_geno_gram's exact integers and the fp64 restatement of tests/_quantgen.py.  Needs an MI355X.

Shapes: n in {1, 2, 33, 129, 257} (a lone tile, a partial diagonal tile, a partial off-diagonal
tile of the 128 x 128 tiling), L in {1, 70, 1000, 2500} (padding bits; fp32 chains of 1024 loci
crossed twice with a remainder).

Exact anchor: with val[l] = {0, 1, 2} the sums are integers of at most 4 * 1024 < 2^24 per fp32
chain, so gnx_grm must equal gnx_geno_gram exactly.  Weighted: |G_ij - ref| <= (1.01 * 1024 *
2^-24 + L * 2^-53) * sum_l |v_il v_jl| against fp64 numpy on the same fp32 table (a first-order
bound of an fma chain of at most 1024 products, then an fp64 sum).  Observed on the MI355X (the
printed `ratio`): at most 0.13 of that bound (the dominance table at n = 257, L = 1000, whose
rare alleles carry large values), 0.03 for the GCTA table at n >= 33 and 0.02 for a random table:
the sqrt(1024) / 1024 of rounding errors that add like a random walk, and its tail over n^2
entries.

Model level (about 320 individuals, 1000 loci), against the restatement on get_genotypes, 1e-6
absolute in the Trait's units (sd(z) = 0.072): observed gaps h2 1.4e-10 (z, at the boundary) and
4.0e-7 (z plus noise), g_hat 1.4e-8 (z), 2.2e-7 (z plus noise), 4.2e-7 (two thirds trained)."""
import numpy as np
import pytest

import _quantgen as QT
from test_gpu_parity import native

pytestmark = pytest.mark.gpu

N_ALL = 257
NS = [1, 2, 33, 129, 257]
LS = [1, 70, 1000, 2500]


def _dosages(packed, L):
    """dosages int64 [n][L] of packed genomes uint64 [n][2][W64]"""
    b = np.unpackbits(np.ascontiguousarray(packed).view(np.uint8), axis=-1, bitorder='little')
    return b[:, 0, :L].astype(np.int64) + b[:, 1, :L]


def _mask(loci, W64):
    m = np.zeros(W64, np.uint64)
    np.bitwise_or.at(m, loci >> 6, np.uint64(1) << (loci & 63).astype(np.uint64))
    return m


_DEVS = {}


@pytest.fixture(scope='module')
def devs():
    """L -> (handle with 257 individuals of random genotypes, their dosages), made on demand"""
    import gnx_oracle as O
    nat = native()

    def get(L):
        if L not in _DEVS:
            rng = np.random.RandomState(100 + L)
            p = rng.uniform(0.03, 0.97, L)
            gts = (rng.rand(N_ALL, L, 2) < p[None, :, None]).astype(np.uint8)
            dev = nat.Device(16, 16, 1, L=L, n_traits=0, cap_inds=N_ALL + 64,
                             cap_rows=N_ALL + 64, seed=3)
            dev.upload_rasters(np.ones((1, 16, 16), np.float32))
            dev.set_species_params(nat.default_species_params())
            dev.upload_population(rng.rand(N_ALL) * 16, rng.rand(N_ALL) * 16, np.zeros(N_ALL),
                                  np.zeros(N_ALL), np.arange(N_ALL))
            dev.upload_genomes(O.pack_genomes(gts))
            D = _dosages(dev.download_genomes(np.arange(N_ALL)), L)
            np.testing.assert_array_equal(D, gts.sum(2))
            _DEVS[L] = (dev, D)
        return _DEVS[L]

    yield get
    for dev, _ in _DEVS.values():
        dev.close()
    _DEVS.clear()


def _val012(L):
    return np.tile(np.arange(3, dtype=np.float32), (L, 1))


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('L', LS)
def test_exact_anchor_symmetry_and_repeatability(devs, L, n):
    dev, D = devs(L)
    rng = np.random.RandomState(7 * L + n)
    slots = rng.choice(N_ALL, n, replace=False).astype(np.int64)
    G = dev.grm(_val012(L), slots)
    assert G.dtype == np.float64 and G.shape == (n, n)
    ref = dev.geno_gram(slots)
    np.testing.assert_array_equal(G, ref.astype(np.float64))
    np.testing.assert_array_equal(ref, D[slots] @ D[slots].T)
    np.testing.assert_array_equal(G, G.T)
    np.testing.assert_array_equal(dev.grm(_val012(L), slots), G)       # bit-equal again
    info = dev.grm_info()
    T = (n + 127) // 128
    assert info['tiles'] == T * (T + 1) // 2 and info['kernel_ms'] > 0
    assert info['k_chunks'] == ((L + 63) // 64 + 15) // 16


@pytest.mark.parametrize('L', [1000, 2500])
def test_exact_anchor_under_a_mask_with_empty_words_and_descending_slots(devs, L):
    dev, D = devs(L)
    rng = np.random.RandomState(L)
    loci = np.sort(rng.choice(L, L // 3, replace=False))
    loci = loci[((loci >> 6) % 3 != 1) & ((loci >> 6) != 0)]        # whole words left empty
    loci = np.union1d(loci, [L - 1])                                 # next to the padding
    mask = _mask(loci, dev.W64)
    assert (mask == 0).sum() >= dev.W64 // 3
    for slots in (np.arange(N_ALL)[::-1].copy(), np.arange(140, 7, -1), None):
        G = dev.grm(_val012(L), slots, mask)
        ref = dev.geno_gram(slots, mask)
        np.testing.assert_array_equal(G, ref.astype(np.float64))
        rows = np.arange(N_ALL) if slots is None else slots
        np.testing.assert_array_equal(ref, D[rows][:, loci] @ D[rows][:, loci].T)
    # a table that is non-zero everywhere: what the mask leaves out must not be selected
    val = _val012(L) + 5.0
    G = dev.grm(val, None, mask)
    Z = D[:, loci] + 5.0
    np.testing.assert_array_equal(G, Z @ Z.T)                         # integers below 2^24


def test_exact_anchor_on_an_uncompacted_population_with_a_pending_crossover():
    """the product path (lazy mortality between the steps of a walk, the crossover launched
    behind the next step): gnx_grm joins the crossover and gathers the living before it reads"""
    from test_gpu_product_path import _make, _paths, L as PP_L
    dev, _ = _make(_paths(False), cap_inds=1 << 20, cap_rows=1 << 15, N=12000, K_factor=8.0)
    try:
        dev.walk(4, False, True)
        pc = dev.path_counts()
        assert pc['lazy_mortalities'] > 0 and pc['xo_launch_p2'] > 0, pc
        slots = np.random.RandomState(4).choice(8000, 257, replace=False).astype(np.int64)
        G = dev.grm(_val012(PP_L), slots)                 # first: the handle as the walk left it
        assert dev.N >= 8000
        np.testing.assert_array_equal(G, dev.geno_gram(slots).astype(np.float64))
        D = _dosages(dev.download_genomes(slots), PP_L)
        np.testing.assert_array_equal(G, D @ D.T)
        assert dev.grm_info()['k_chunks'] == 98           # 1563 words in chains of 16
    finally:
        dev.close()


RATIOS = {}


@pytest.mark.parametrize('table', ['random', 'gcta', 'dominance'])
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('L', LS)
def test_weighted_within_the_derived_bound(devs, L, n, table):
    dev, D = devs(L)
    rng = np.random.RandomState(11 * L + n)
    slots = rng.choice(N_ALL, n, replace=False).astype(np.int64)
    Ds = D[slots]
    mask, used = None, np.ones(L, bool)
    if table == 'random':
        val = rng.standard_normal((L, 3)).astype(np.float32)
    else:
        from geonomics_amd.sim import quantgen as Q
        kind = 'additive' if table == 'gcta' else 'dominance'
        val, used = Q.grm_values(Ds.sum(0), n, kind, min_maf=0.0)
        mask = _mask(np.flatnonzero(used), dev.W64)        # (empty for some n = 1 or L = 1: G = 0)
        val = val + np.float32(np.where(used, 0.0, 7.0))[:, None]     # never to be selected
    G = dev.grm(val, slots, mask)
    Z = QT.expand(val.astype(np.float64), Ds)[:, used]
    ref = Z @ Z.T
    bound = QT.grm_bound(np.abs(Z), L)
    err = np.abs(G - ref)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    RATIOS[(L, n, table)] = ratio
    print('grm L %d n %d %s: max |err| %.3g, ratio to the bound %.4f' % (L, n, table, err.max(),
                                                                      ratio))
    assert (err <= bound).all()
    np.testing.assert_array_equal(G, G.T)
    np.testing.assert_array_equal(dev.grm(val, slots, mask), G)
    if table == 'gcta' and n >= 33 and L >= 1000:
        assert abs(np.diag(G).mean() - np.diag(ref).mean()) < 1e-3


def test_refusals(devs):
    nat = native()
    dev, _ = devs(70)
    val = _val012(70)
    with pytest.raises(nat.GnxError, match='gnx_grm: 1..8192 individuals'):
        dev.grm(val, np.zeros(0, np.int64))
    with pytest.raises(nat.GnxError, match='gnx_grm: 1..8192 individuals'):
        dev.grm(val, np.arange(8193))
    with pytest.raises(nat.GnxError, match='slot out of range'):
        dev.grm(val, np.array([0, N_ALL]))
    with pytest.raises(ValueError, match='val: shape'):
        dev.grm(val[:-1], np.arange(3))
    with pytest.raises(ValueError, match='locus_mask'):
        dev.grm(val, np.arange(3), np.zeros(5, np.uint64))
    bare = nat.Device(16, 16, 1, L=70, cap_inds=64, cap_rows=64, seed=1)
    bare.upload_rasters(np.ones((1, 16, 16), np.float32))
    bare.set_species_params(nat.default_species_params())
    bare.upload_population(np.ones(4), np.ones(4), np.zeros(4), np.zeros(4), np.arange(4))
    with pytest.raises(nat.GnxError, match='gnx_grm: genomes not assigned'):
        bare.grm(val)
    bare.close()


# ------------------------------------------------------------------ the Model
@pytest.fixture(scope='module')
def model():
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    mod = gnx.make_model(small_params(seed=5, L=1000))
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(12, 'main', verbose=False)
    return mod


def test_model_calls_equal_the_restatement(model):
    mod = model
    spp = mod.comm[0]
    ids = np.array([*spp])
    n = ids.size
    assert 250 < n < 400
    D = np.rint(mod.get_genotypes() * 2).astype(np.int64)           # ids ascending
    z = np.asarray(spp._get_z(0), np.float64).ravel()
    res = mod.calc_grm()
    Gref, used, Z = QT.grm_from_dosages(D)
    np.testing.assert_array_equal(res['ids'], ids)
    np.testing.assert_array_equal(res['loci_used'], np.flatnonzero(used))
    assert res['n_loci'] == used.sum() > 500 and res['kernel_ms'] > 0
    np.testing.assert_array_equal(res['p'], D.sum(0)[used] / (2.0 * n))
    err, bound = np.abs(res['G'] - Gref), QT.grm_bound(np.abs(Z), 1000)
    print('model G: max |err| %.3g, ratio to the bound %.4f' % (err.max(), (err / bound).max()))
    assert (err <= bound).all()
    np.testing.assert_array_equal(res['G'], res['G'].T)
    assert abs(np.diag(res['G']).mean() - np.diag(Gref).mean()) < 1e-3
    X1 = np.ones((n, 1))
    rng = np.random.RandomState(9)
    # z plus noise of z's own variance, in the Trait's units: the 1e-6 below is absolute, so it
    # belongs to a scale, and the scale it is stated for is the Trait's phenotype.  (With this
    # response standardised to variance 2, g_hat scales by 1 / sd(z) and its gap with it: 3.4e-6
    # was observed, 2.4e-6 of sd(y), which is what G's fp32 rounding of 1.9e-6 per entry gives
    # through V^-1 and through the shift of 2e-6 in ln delta that it causes.)
    y = z + z.std() * rng.standard_normal(n)
    print('model: sd(z) %.4f' % z.std())
    gaps = {}
    for name, resp, kw in (('z', z, {}), ('z + noise', y, dict(y=y))):
        h = mod.calc_heritability(0, **kw)
        ref = QT.reml_brute(Gref, resp, X1)
        print('model %s: h2 %.9f restated %.9f (gap %.3g), logL %.9f restated %.9f, se %.4f, '
              'he %.4f, boundary %s' % (name, h['h2'], ref['h2'], abs(h['h2'] - ref['h2']),
                                        h['logL'], ref['logL'], h['se_h2'], h['he_h2'],
                                        h['at_boundary']))
        gaps['h2 of ' + name] = abs(h['h2'] - ref['h2'])
        # (the same arithmetic on the device's own matrix: Haseman-Elston is not iterative)
        assert h['he_h2'] == pytest.approx(QT.he_dense(res['G'], resp, X1), rel=1e-9, abs=1e-12)
        assert h['n_loci'] == res['n_loci'] and (h['ids'] == ids).all()
        shared = mod.calc_heritability(0, grm=res, **kw)
        for k in ('h2', 'Vg', 'Ve', 'logL', 'he_h2', 'delta'):
            assert shared[k] == h[k], k
        pb = mod.predict_breeding_values(0, grm=res, **kw)
        g_ref, _ = QT.blup_dense(Gref, resp, X1, ref['delta'])
        gaps['g_hat of ' + name] = np.abs(pb['g_hat'] - g_ref).max()
        assert pb['h2'] == h['h2']
    # two thirds trained: the rest predicted, and the accuracy against the Trait's true z
    train = ids[np.arange(n) % 3 != 0]
    pt = mod.predict_breeding_values(0, train=train)
    tix = np.flatnonzero(np.arange(n) % 3 != 0)
    sub = QT.reml_brute(Gref[np.ix_(tix, tix)], z[tix], X1[tix])
    g_ref, _ = QT.blup_dense(Gref, z, X1, sub['delta'], tix)
    gaps['h2 of the trained'] = abs(pt['h2'] - sub['h2'])
    gaps['g_hat from the trained'] = np.abs(pt['g_hat'] - g_ref).max()
    print('model train: h2 %.9f restated %.9f, accuracy %.4f' % (pt['h2'], sub['h2'],
                                                                pt['accuracy']))
    print('model gaps: ' + ', '.join('%s %.3g' % kv for kv in gaps.items()))
    assert all(v <= 1e-6 for v in gaps.values()), gaps
    rest = np.setdiff1d(np.arange(n), tix)
    assert pt['accuracy'] == pytest.approx(np.corrcoef(pt['g_hat'][rest], z[rest])[0, 1])
    np.testing.assert_array_equal(pt['train'], train)
    # a sample, a subset of loci and the other weightings go through
    sub = mod.calc_grm(n=100, loci=np.arange(200, 900), method='vanraden')
    assert sub['G'].shape == (100, 100) and sub['loci_used'].min() >= 200
    o = np.searchsorted(ids, sub['ids'])
    val, u2 = QT.table_direct(np.where((np.arange(1000) >= 200) & (np.arange(1000) < 900),
                                       D[o].sum(0), 0), 100, method='vanraden')
    Zs = QT.expand(val.astype(np.float32).astype(np.float64), D[o])
    assert (np.abs(sub['G'] - Zs @ Zs.T) <= QT.grm_bound(np.abs(Zs), 1000)).all()


def test_model_refusals(model):
    from geonomics_amd.structs.tiled import TiledSpecies
    mod = model
    with pytest.raises(ValueError, match="kind: 'additive' or 'dominance'"):
        mod.calc_grm(kind='x')
    with pytest.raises(ValueError, match='y: finite values'):
        mod.calc_heritability(y=np.ones(3))
    with pytest.raises(ValueError, match='give individs or n, not both'):
        mod.calc_grm(individs=[1], n=2)
    for name in ('_calc_grm', '_calc_heritability', '_predict_breeding_values'):
        with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
            getattr(TiledSpecies, name)(mod.comm[0])
