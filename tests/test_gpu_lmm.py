"""The per-locus quadratic forms of the mixed-model scan on the device (csrc/gnx_quad.hip: f32
MFMA over the individuals, fp64 sums of squares) through the C-ABI (Device.assoc_quad) and through
the Model (run_lmm), against exact integers and the fp64 restatements of tests/_lmm.py.  Needs an
MI355X.

Shapes: n in {1, 2, 33, 129, 257} (a lone ragged stage of 32 individuals; several; more than 128
columns of M), m in {1, 33, 129, n} (one ragged and two tiles of 128 rows of M), L in {1, 70, 1000,
2500} (a lone word beside the padding word of its locus tile, padding bits, several locus tiles),
and n in {1025, 2081}: one and two flushes of the fp32 chains after 1024 individuals, then a
ragged stage.

Exact anchors: with val[l] = {0, 1, 2} and small integers in M every C_kl is an integer below
2^24 and every sum of squares one below 2^53, so q must equal the int64 numpy value exactly.
Weighted: |q - ref| <= the bound of include/gnx_hip.h, computed from the fp64 restatement on the
same fp32 inputs.  Observed on the MI355X (the printed `ratio`): at most 0.023 of that bound (a
real rotation at n = 33, L = 1000), 0.019 for a random normal M at n = 33, 0.0001 to 0.002 at
n >= 257: the rows' errors are independent, the bound adds them as if they were not."""
import ctypes as C

import numpy as np
import pytest

import _lmm as LT
import _quantgen as QT
from test_gpu_parity import native
from test_gpu_quantgen import _dosages, _mask, _val012

pytestmark = pytest.mark.gpu

N_ALL = 257
N_BIG = 2081
NS = [1, 2, 33, 129, 257]
LS = [1, 70, 1000, 2500]

_DEVS = {}


@pytest.fixture(scope='module')
def devs():
    """(L, N) -> (handle with N individuals of random genotypes, their dosages), made on demand"""
    import gnx_oracle as O
    nat = native()

    def get(L, N=N_ALL):
        if (L, N) not in _DEVS:
            rng = np.random.RandomState(100 + L + N)
            p = rng.uniform(0.03, 0.97, L)
            gts = (rng.rand(N, L, 2) < p[None, :, None]).astype(np.uint8)
            dev = nat.Device(16, 16, 1, L=L, n_traits=0, cap_inds=N + 64, cap_rows=N + 64, seed=3)
            dev.upload_rasters(np.ones((1, 16, 16), np.float32))
            dev.set_species_params(nat.default_species_params())
            dev.upload_population(rng.rand(N) * 16, rng.rand(N) * 16, np.zeros(N), np.zeros(N),
                                  np.arange(N))
            dev.upload_genomes(O.pack_genomes(gts))
            _DEVS[(L, N)] = (dev, gts.sum(2).astype(np.int64))
        return _DEVS[(L, N)]

    yield get
    for dev, _ in _DEVS.values():
        dev.close()
    _DEVS.clear()


def _q_int(M, Z):
    Cm = M.astype(np.int64) @ Z.astype(np.int64)
    return (Cm * Cm).sum(axis=0)


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('L', LS)
def test_exact_integer_anchor_and_repeatability(devs, L, n):
    dev, D = devs(L)
    rng = np.random.RandomState(7 * L + n)
    slots = rng.choice(N_ALL, n, replace=False).astype(np.int64)
    for m in sorted({1, 33, 129, n}):
        M = rng.randint(-2, 3, (m, n))
        got = dev.assoc_quad(_val012(L), M, slots)
        q = got['q']
        assert q.dtype == np.float64 and q.shape == (L,) and got['kernel_ms'] > 0
        ref = _q_int(M, D[slots])
        assert np.abs(M @ D[slots]).max() < 2 ** 24 and ref.max() < 2 ** 53
        np.testing.assert_array_equal(q, ref.astype(np.float64))
        assert dev.assoc_quad(_val012(L), M, slots)['q'].tobytes() == q.tobytes()


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('L', LS)
def test_identity_anchor_gives_the_second_moment(devs, L, n):
    dev, D = devs(L)
    slots = np.random.RandomState(3 * L + n).choice(N_ALL, n, replace=False).astype(np.int64)
    q = dev.assoc_quad(_val012(L), np.eye(n), slots)['q']
    s2 = dev.assoc_cross(np.ones(n), slots)['s2']
    np.testing.assert_array_equal(q, s2.astype(np.float64))
    np.testing.assert_array_equal(s2, (D[slots] ** 2).sum(0))


@pytest.mark.parametrize('n', [33, 129])
@pytest.mark.parametrize('L', [70, 1000])
def test_trace_of_the_grm_equals_the_sum_of_the_identity_forms(devs, L, n):
    """the two users of the shared f32 MFMA tile on one handle and one table: trace(G) and the sum
    of q under M = I are both sum_i sum_l val[l][d_il]^2, an integer below 2^53 (at most
    129 * 1000 * 49), whichever of the two reductions (over the loci, over the individuals) ran"""
    dev, D = devs(L)
    rng = np.random.RandomState(11 * L + n)
    slots = rng.choice(N_ALL, n, replace=False).astype(np.int64)
    loci = np.union1d(np.sort(rng.choice(L, L // 2, replace=False)), [L - 1])
    for val, shift in ((_val012(L), 0), (_val012(L) + 5.0, 5)):
        for mask, used in ((None, np.arange(L)), (_mask(loci, dev.W64), loci)):
            ref = int(((D[slots][:, used] + shift) ** 2).sum())
            assert 0 < ref < 2 ** 53
            tr = np.trace(dev.grm(val, slots, mask))
            qs = dev.assoc_quad(val, np.eye(n), slots, mask)['q'].sum()
            assert tr == qs == float(ref)


@pytest.mark.parametrize('n', [1025, 2081])
def test_exact_across_the_flushes_of_the_fp32_chains(devs, n):
    dev, D = devs(70, N_BIG)
    rng = np.random.RandomState(n)
    slots = rng.choice(N_BIG, n, replace=False).astype(np.int64)
    M = rng.randint(-1, 2, (33, n))
    q = dev.assoc_quad(_val012(70), M, slots)['q']
    np.testing.assert_array_equal(q, _q_int(M, D[slots]).astype(np.float64))
    # every chain of 1024 individuals on its own, and the ragged rest: the flushes add them
    parts = [(M[:, a:a + 1024].astype(np.int64) @ D[slots][a:a + 1024]) for a in range(0, n, 1024)]
    assert len(parts) == (n + 1023) // 1024 and all(np.abs(p).max() > 0 for p in parts)
    np.testing.assert_array_equal(q, (sum(parts) ** 2).sum(0).astype(np.float64))


@pytest.mark.parametrize('L', [1000, 2500])
def test_exact_under_a_mask_with_empty_words_and_descending_slots(devs, L):
    dev, D = devs(L)
    rng = np.random.RandomState(L)
    loci = np.sort(rng.choice(L, L // 3, replace=False))
    loci = loci[((loci >> 6) % 3 != 1) & ((loci >> 6) != 0)]        # whole words left empty
    loci = np.union1d(loci, [L - 1])                                 # next to the padding
    mask = _mask(loci, dev.W64)
    assert (mask == 0).sum() >= dev.W64 // 3
    out = np.setdiff1d(np.arange(L), loci)
    # a table that is non-zero everywhere: what the mask leaves out must not be selected
    val = _val012(L) + 5.0
    for slots in (np.arange(N_ALL)[::-1].copy(), np.arange(140, 7, -1), None):
        rows = np.arange(N_ALL) if slots is None else slots
        M = rng.randint(-2, 3, (33, rows.size))
        q = dev.assoc_quad(val, M, slots, mask)['q']
        ref = _q_int(M, D[rows] + 5)
        np.testing.assert_array_equal(q[loci], ref[loci].astype(np.float64))
        assert q[out].tobytes() == np.zeros(out.size).tobytes()     # exactly +0


def test_exact_on_an_uncompacted_population_with_a_pending_crossover():
    """the product path (lazy mortality between the steps of a walk, the crossover launched
    behind the next step): gnx_assoc_quad joins the crossover and gathers the living first"""
    from test_gpu_product_path import _make, _paths, L as PP_L
    dev, _ = _make(_paths(False), cap_inds=1 << 20, cap_rows=1 << 15, N=12000, K_factor=8.0)
    try:
        dev.walk(4, False, True)
        pc = dev.path_counts()
        assert pc['lazy_mortalities'] > 0 and pc['xo_launch_p2'] > 0, pc
        rng = np.random.RandomState(4)
        slots = rng.choice(8000, 257, replace=False).astype(np.int64)
        M = rng.randint(-2, 3, (33, 257))
        loci = np.arange(0, PP_L, 37)
        q = dev.assoc_quad(_val012(PP_L), M, slots, _mask(loci, dev.W64))['q']   # first: as walked
        assert dev.N >= 8000
        D = _dosages(dev.download_genomes(slots), PP_L)
        ref = np.zeros(PP_L)
        ref[loci] = _q_int(M, D)[loci]
        np.testing.assert_array_equal(q, ref)
    finally:
        dev.close()


RATIOS = {}


@pytest.mark.parametrize('form', ['normal', 'rotation'])
@pytest.mark.parametrize('n', [33, 257, 1025])
@pytest.mark.parametrize('L', [70, 1000])
def test_weighted_within_the_derived_bound(devs, L, n, form):
    from geonomics_amd.sim import assoc as A
    dev, D = devs(L, N_BIG)
    rng = np.random.RandomState(13 * L + n)
    slots = rng.choice(N_BIG, n, replace=False).astype(np.int64)
    Ds = D[slots]
    s1, s2 = Ds.sum(0), (Ds * Ds).sum(0)
    use, _ = A.lmm_testable(s1, s2, n, 0.0)
    val = A.lmm_table(s1, n, use)
    if form == 'normal':
        M = rng.standard_normal((n, n)).astype(np.float32)
    else:
        evals, U = np.linalg.eigh(LT.grm_dense(Ds, min_maf=0.0))
        M = A.lmm_rotation(evals, U, 1.0).astype(np.float32)
    mask = _mask(np.flatnonzero(use), dev.W64)
    val7 = val + np.float32(np.where(use, 0.0, 7.0))[:, None]         # never to be selected
    q = dev.assoc_quad(val7, M, slots, mask)['q']
    ref, Cm, S = LT.quad_ref(val, M, Ds, use)
    bound = LT.quad_bound(Cm, S, n)
    err = np.abs(q - ref)
    ok = bound > 0
    ratio = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
    RATIOS[(L, n, form)] = ratio
    print('quad L %d n %d %s: max |err| %.3g of q %.3g, ratio to the bound %.4f'
          % (L, n, form, err.max(), ref.max(), ratio))
    assert use.sum() > L // 2 and (err <= bound).all()
    assert (q[~use] == 0).all()
    assert dev.assoc_quad(val7, M, slots, mask)['q'].tobytes() == q.tobytes()


def test_refusals_launch_nothing(devs):
    nat = native()
    dev, _ = devs(70)
    val = _val012(70)
    slots = np.arange(5, dtype=np.int64)
    M = np.arange(15, dtype=np.float32).reshape(3, 5)
    before = dev.assoc_quad(val, M, slots)['q']

    def refused(match, val_=val, M_=M, slots_=slots):
        with pytest.raises(nat.GnxError, match=match):
            dev.assoc_quad(val_, M_, slots_)

    refused('gnx_assoc_quad: 1..8192 individuals', M_=np.zeros((3, 0)), slots_=np.zeros(0, np.int64))
    refused('gnx_assoc_quad: 1..8192 individuals', M_=np.zeros((1, 8193)),
            slots_=np.zeros(8193, np.int64))
    refused(r'1 <= m <= 8192 rows of M \(got 0\)', M_=np.zeros((0, 5)))
    refused(r'1 <= m <= 8192 rows of M \(got 8193\)', M_=np.zeros((8193, 5)))
    for bad in (np.nan, np.inf, -np.inf):
        Mb = M.copy()
        Mb[2, 4] = bad
        refused(r'M is not finite \(row 2, column 4\)', M_=Mb)
        vb = val.copy()
        vb[69, 1] = bad
        refused(r'val is not finite \(locus 69\)', val_=vb)
    refused('slot out of range', slots_=np.array([0, 1, 2, 3, N_ALL]))
    refused('slot out of range', slots_=np.array([0, 1, 2, 3, -1]))
    with pytest.raises(nat.GnxError, match=r'n = 5 but %d individuals are alive' % N_ALL):
        q = np.zeros(70)
        dev._chk(dev.lib.gnx_assoc_quad(
            dev.h, C.c_int64(5), None, None, val.ctypes.data_as(C.POINTER(C.c_float)),
            C.c_int32(3), M.ctypes.data_as(C.POINTER(C.c_float)),
            q.ctypes.data_as(C.POINTER(C.c_double)), None))
    for null in ('val', 'M', 'q'):
        q = np.zeros(70)
        args = dict(val=val.ctypes.data_as(C.POINTER(C.c_float)),
                    M=M.ctypes.data_as(C.POINTER(C.c_float)),
                    q=q.ctypes.data_as(C.POINTER(C.c_double)))
        args[null] = None
        with pytest.raises(nat.GnxError, match='null table, M or output'):
            dev._chk(dev.lib.gnx_assoc_quad(
                dev.h, C.c_int64(5), slots.ctypes.data_as(C.POINTER(C.c_int64)), None,
                args['val'], C.c_int32(3), args['M'], args['q'], None))
    with pytest.raises(ValueError, match='val: shape'):
        dev.assoc_quad(val[:-1], M, slots)
    with pytest.raises(ValueError, match=r'M: .* not \[m\]\[n = 5\]'):
        dev.assoc_quad(val, M[:, :-1], slots)
    with pytest.raises(ValueError, match='locus_mask'):
        dev.assoc_quad(val, M, slots, np.zeros(5, np.uint64))
    assert dev.assoc_quad(val, M, slots)['q'].tobytes() == before.tobytes()
    # an empty mask: zeros, nothing to launch
    empty = dev.assoc_quad(val, M, slots, np.zeros(dev.W64, np.uint64))
    assert not empty['q'].any() and empty['kernel_ms'] == 0.0
    # a handle whose genomes were never assigned, and one that holds ghost records
    bare = nat.Device(16, 16, 1, L=70, cap_inds=64, cap_rows=64, seed=1)
    try:
        bare.upload_rasters(np.ones((1, 16, 16), np.float32))
        bare.set_species_params(nat.default_species_params())
        bare.upload_population(np.ones(4), np.ones(4), np.zeros(4), np.zeros(4), np.arange(4))
        with pytest.raises(nat.GnxError, match='gnx_assoc_quad: genomes not assigned'):
            bare.assoc_quad(val, np.ones((2, 4)))
    finally:
        bare.close()
    import gnx_oracle as O
    tile = nat.Device(16, 16, 1, L=70, n_traits=0, cap_inds=64, cap_rows=64, seed=1)
    try:
        tile.upload_rasters(np.ones((1, 16, 16), np.float32))
        tile.set_species_params(nat.default_species_params())
        tile.upload_population(np.ones(4), np.ones(4), np.zeros(4), np.zeros(4), np.arange(4))
        tile.upload_genomes(O.pack_genomes(np.ones((4, 70, 2), np.uint8)))
        assert (tile.assoc_quad(val, np.ones((2, 4)))['q'] == 2 * 8.0 ** 2).all()
        rec = np.zeros(1, nat.IND_REC)
        rec['x'], rec['y'], rec['id'] = 1.0, 1.0, 10 ** 6
        tile.tile_import_ghosts(rec)
        with pytest.raises(nat.GnxError, match='gnx_assoc_quad: the handle holds ghost records'):
            tile.assoc_quad(val, np.ones((2, 4)))
    finally:
        tile.close()


# ------------------------------------------------------------------ the Model
# beta and t of run_lmm against the dense fp64 restatement on get_genotypes, t relative to
# max(|t|, 1) and beta to max(|beta|, se): the gap is the fp32 rounding of G (through delta and
# the rotation), of the rotation handed to the device and of q, carried through
# gg = q - sum (z . A_j)^2; it does not follow from the kernel's bound alone.  Observed on the
# MI355X: 1.88e-6 (t) and 1.86e-6 (beta) without covariates, 1.82e-6 and 1.82e-6 with two; the
# tolerance is 5.3 times the largest.
MODEL_TOL = 1e-5


@pytest.fixture(scope='module')
def model():
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    mod = gnx.make_model(small_params(seed=5, L=1000))
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(12, 'main', verbose=False)
    return mod


def _response(mod):
    spp = mod.comm[0]
    ids = np.array([*spp])
    z = np.asarray(spp._get_z(0), np.float64).ravel()
    rng = np.random.RandomState(9)
    return ids, z + z.std() * rng.standard_normal(ids.size)


def _rel_gaps(res, ref, tested):
    """the largest gaps of t, relative to max(|t|, 1), and of beta, relative to max(|beta|, se)
    (the same scale: beta / se = t)"""
    t, b = res['t'][tested, 0], res['beta'][tested, 0]
    rt, rb, rs = ref['t'][tested], ref['beta'][tested], ref['se'][tested]
    return (float((np.abs(t - rt) / np.maximum(np.abs(rt), 1.0)).max()),
            float((np.abs(b - rb) / np.maximum(np.abs(rb), rs)).max()))


def test_run_lmm_equals_the_dense_restatement(model):
    from geonomics_amd.sim import assoc as A
    mod = model
    ids, y = _response(mod)
    n = ids.size
    assert 250 < n < 400
    D = np.rint(mod.get_genotypes() * 2).astype(np.int64)           # ids ascending
    covar = np.random.RandomState(2).standard_normal((n, 2))
    gaps = []
    for kw, Cc in ((dict(), None), (dict(covars=covar), covar)):
        res = mod.run_lmm(y=y, **kw)
        h = mod.calc_heritability(y=y, **kw)
        assert res['delta'] == h['delta'] and res['h2'] == h['h2']
        assert res['Vg'] == h['Vg'] and res['Ve'] == h['Ve']
        assert res['at_boundary'] == h['at_boundary'] and res['n_loci_grm'] == h['n_loci']
        assert set(res['seconds']) == {'grm', 'eigh', 'reml', 'quad', 'cross'}
        assert res['kernel_ms'] > 0 and res['trait_loci'] is None
        np.testing.assert_array_equal(res['ids'], ids)
        np.testing.assert_array_equal(res['loci'], np.arange(1000))
        Gref, used, _ = QT.grm_from_dosages(D)
        assert res['n_loci_grm'] == used.sum()
        ref = LT.lmm_brute(D, y, Cc, Gref, res['delta'])
        s1, s2 = D.sum(0), (D * D).sum(0)
        use, maf = A.lmm_testable(s1, s2, n)
        np.testing.assert_array_equal(res['tested'], use)
        np.testing.assert_array_equal(res['maf'], maf)
        assert res['df'] == ref['df'] and use.sum() > 500
        gt, gb = _rel_gaps(res, ref, use)
        print('run_lmm covars %s: delta %.6g h2 %.4f gif %.3f, gap t %.3g beta %.3g'
              % (Cc is not None, res['delta'], res['h2'], res['gif'][0], gt, gb))
        assert np.isnan(res['t'][~use]).all()
        gaps += [gt, gb]
    assert max(gaps) <= MODEL_TOL, gaps


def test_run_lmm_reuse_limits_and_refusals(model):
    from geonomics_amd.sim import quantgen as Q
    from geonomics_amd.structs.tiled import TiledSpecies
    mod = model
    ids, y = _response(mod)
    n = ids.size
    fresh = mod.run_lmm(y=y)
    grm = mod.calc_grm()
    assert 'eig' not in grm
    shared = mod.run_lmm(y=y, grm=grm)
    assert 'eig' in grm and shared['seconds']['grm'] == 0.0
    for k in ('beta', 'se', 't', 'p', 'q', 'maf', 'tested', 'gif'):
        np.testing.assert_array_equal(shared[k], fresh[k], err_msg=k)
    assert shared['delta'] == fresh['delta']
    again = mod.run_lmm(y=y, grm=grm)                                # the kept eigendecomposition
    assert again['seconds']['eigh'] == 0.0
    np.testing.assert_array_equal(again['t'], fresh['t'])
    # the Trait's own phenotype, and a selection of rows
    byz = mod.run_lmm(0, grm=grm, loci=[5, 17, 900])
    assert byz['t'].shape == (3, 1) and byz['trait_loci'] is not None
    np.testing.assert_array_equal(byz['loci'], [5, 17, 900])
    # a huge delta is the OLS scan: the host limit of tests/test_lmm_host.py plus the gap above
    big = mod.run_lmm(y=y, grm=grm, delta=1e12)
    ols = mod.run_gwas(y=y)
    assert big['delta'] == 1e12 and np.isnan(big['h2']) and big['at_boundary'] is False
    np.testing.assert_array_equal(big['tested'], ols['tested'])
    tt = big['tested']
    gap = float((np.abs(big['t'][tt] - ols['t'][tt]) / np.maximum(np.abs(ols['t'][tt]), 1.0)).max())
    lim = 100.0 * grm['eig'][0].max() / 1e12 + MODEL_TOL
    print('run_lmm delta 1e12 against run_gwas: gap %.3g, limit %.3g' % (gap, lim))
    assert gap <= lim
    # grm_loci changes the matrix, not what is tested
    part = mod.run_lmm(y=y, grm_loci=np.arange(200, 900))
    assert 0 < part['n_loci_grm'] < fresh['n_loci_grm']
    assert part['n_loci_grm'] == mod.calc_grm(loci=np.arange(200, 900))['n_loci']
    np.testing.assert_array_equal(part['tested'], fresh['tested'])
    np.testing.assert_array_equal(part['loci'], fresh['loci'])
    assert part['delta'] != fresh['delta']
    # refusals
    for bad in (0.0, -2.0, np.nan, np.inf, True):
        with pytest.raises(ValueError, match='run_lmm: delta: a positive, finite'):
            mod.run_lmm(y=y, delta=bad)
    with pytest.raises(ValueError, match='run_lmm: one response y'):
        mod.run_lmm(y=np.column_stack([y, y]))
    with pytest.raises(ValueError, match='run_lmm: y: finite values'):
        mod.run_lmm(y=y[:-1])
    with pytest.raises(ValueError, match='run_lmm: grm: its ids are not'):
        mod.run_lmm(y=y[:50], individs=ids[:50], grm=grm)
    old = Q.GRM_MAX
    Q.GRM_MAX = n - 1
    try:
        with pytest.raises(ValueError, match=r'run_lmm: at most %d individuals \(the relationship '
                                             r'matrix is n x n\), got %d' % (n - 1, n)):
            mod.run_lmm(y=y)
    finally:
        Q.GRM_MAX = old
    traits = mod.comm[0].gen_arch.traits
    mod.comm[0].gen_arch.traits = {}
    try:
        with pytest.raises(ValueError, match='run_lmm: the Species has no Traits; give y'):
            mod.run_lmm()
    finally:
        mod.comm[0].gen_arch.traits = traits
    with pytest.raises(NotImplementedError, match='run_lmm with a Species tiled over several GPUs'):
        TiledSpecies._run_lmm(mod.comm[0])
