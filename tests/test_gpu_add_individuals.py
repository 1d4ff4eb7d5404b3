"""Introductions: gnx_transplant (csrc/gnx_transplant.hip), Device.transplant, Species._add_individuals
and Model.add_individuals (reference structs/species.py:1631-2077, sim/model.py:3228-3335).

The device-to-device transplant is pinned bit for bit to the route through the host that the
library already had (download_genomes + tile_import + set_z_range): the same newcomers, columns
and genomes, straight after the call and after further steps with a mutation in between; the
recipient's earlier individuals and the source are untouched; blocks the newcomers shared in the
source are copied once and shared in the recipient, and only a block nobody shares takes a
mutation in place.  Needs an MI355X."""
import numpy as np
import pytest

from test_gpu_parity import native
from test_gpu_product_path import _make, _paths, _slots_of, L as PP_L, NB as PP_NB, W as PP_W, H as PP_H

pytestmark = pytest.mark.gpu

FIRST_ID = 10 ** 7          # above every id a test population reaches
FIT_RTOL = 2e-6             # the project's fitness bar


def _columns(dev, nat):
    """every per-individual column in id order"""
    ids = dev.download(nat.F_ID)
    o = np.argsort(ids, kind='stable')
    return dict(ids=ids[o], x=dev.download(nat.F_X)[o], y=dev.download(nat.F_Y)[o],
                age=dev.download(nat.F_AGE)[o], sex=dev.download(nat.F_SEX)[o],
                fit=dev.download(nat.F_FIT)[o], e=dev.download(nat.F_E)[:, o],
                z=dev.download(nat.F_Z)[:, o])


def _genomes(dev, nat):
    """genomes in id order"""
    ids = dev.download(nat.F_ID)
    return dev.download(nat.F_GENO)[np.argsort(ids, kind='stable')]


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg='%s: %s' % (what, k))


def _halves(dev):
    rows, broken, _, used, free, total = (int(v) for v in dev.debug_halves())
    assert broken == 0 and used + free == total, (broken, used, free, total)
    return dict(rows=rows, used=used, free=free, total=total)


def _walk_source(dev, chunks, rng):
    for c, T in enumerate(chunks):
        dev.walk(T, False, True)
        if c == 0:
            slots = rng.choice(dev.N, 6, replace=False)
            dev.mutate(slots, rng.randint(1, PP_L, 6).astype(np.int32),
                       rng.randint(0, 2, 6).astype(np.uint8))


def _coords(rng, n):
    return ((rng.rand(n) * PP_W * 0.999).astype(np.float32),
            (rng.rand(n) * PP_H * 0.999).astype(np.float32))


@pytest.fixture(scope='module')
def source():
    """a population walked 24 steps (device-driven steps, a mutation in between): many blocks
    of its genomes are shared between relatives"""
    nat = native()
    dev, _ = _make(_paths(False), seed=31, cap_inds=8192, cap_rows=4096)
    _walk_source(dev, (7, 6, 11), np.random.RandomState(5))
    assert dev.N > 1000
    yield dev, nat
    dev.close()


# ------------------------------------------------------------------ 1. against the host-staged route
@pytest.mark.parametrize('large', [False, True], ids=['small_capacity', 'large_capacity'])
def test_transplant_equals_host_staged_route(large, source):
    """A takes 700 individuals through gnx_transplant, its twin B the same 700 through the host
    (gnx_tile_import accepts an untiled handle).  large_capacity: 2^20 slots (lazy mortality,
    the crossover launched behind the next pair list), and the call comes between the births
    and the deaths of a step, when source and recipient still owe their offspring a crossover."""
    nat = native()
    paths = _paths(False)
    caps = dict(cap_inds=1 << 20, cap_rows=1 << 13) if large else dict(cap_inds=8192, cap_rows=4096)
    A, _ = _make(paths, seed=29, **caps)
    B, _ = _make(paths, seed=29, **caps)
    own_src = None
    if large:
        src, _ = own_src = _make(paths, seed=31, **caps)
        _walk_source(src, (7, 6), np.random.RandomState(5))
    else:
        src = source[0]
    try:
        for T in (4, 3):
            for d in (A, B):
                d.walk(T, False, True)
        _assert_same(_columns(A, nat), _columns(B, nat), 'twins before the call')
        np.testing.assert_array_equal(_genomes(A, nat), _genomes(B, nat))
        if large:
            for d in (A, B, src):
                pc = d.path_counts()
                assert pc['lazy_mortalities'] > 0 and pc['xo_launch_p2'] > 0, pc
                d.age()
                d.move()
                d.pop_dynamics_mate(False)
                assert d.counts()[1] > 0
            _assert_same(_columns(A, nat), _columns(B, nat), 'twins after the births')
            for d in (A, src):
                assert d.genome_info()['deferred'] == 1
        rng = np.random.RandomState(17)
        n, N0 = 700, A.N
        assert B.N == N0
        slots = rng.choice(src.N, n, replace=False).astype(np.int64)
        x, y = _coords(rng, n)
        src_before = _columns(src, nat)

        out = A.transplant(src, slots, x, y, FIRST_ID)
        assert out['first_slot'] == N0 and A.N == N0 + n
        assert out['blocks_linked'] == 2 * PP_NB * n
        assert 0 < out['blocks_copied'] <= out['blocks_linked']

        # B: the same newcomers through the host.  (B's state before: its twin's, A's, too.)
        before = _columns(B, nat)
        before_g = _genomes(B, nat)
        assert B.genome_info()['deferred'] == 0          # (reading genomes cut the pending births)
        geno = src.download_genomes(slots)
        rec = np.zeros(n, nat.IND_REC)
        rec['x'], rec['y'] = x, y
        rec['age'] = src.download(nat.F_AGE)[slots]
        rec['sex'] = src.download(nat.F_SEX)[slots]
        rec['id'] = FIRST_ID + np.arange(n)
        rec['fit'] = A.download(nat.F_FIT)[N0:N0 + n]
        B.tile_import(rec, None, geno)
        B.set_z_range(N0, n)

        a, b = _columns(A, nat), _columns(B, nat)
        ga = _genomes(A, nat)
        # the earlier individuals: untouched (the newcomers' ids are above everybody's)
        _assert_same({k: v[..., :N0] for k, v in a.items()}, before, 'earlier individuals')
        np.testing.assert_array_equal(ga[:N0], before_g)
        # the newcomers, in the order of `slots`
        np.testing.assert_array_equal(a['ids'][N0:], FIRST_ID + np.arange(n))
        np.testing.assert_array_equal(a['x'][N0:], x)
        np.testing.assert_array_equal(a['y'][N0:], y)
        np.testing.assert_array_equal(a['age'][N0:], rec['age'])
        np.testing.assert_array_equal(a['sex'][N0:], rec['sex'])
        np.testing.assert_array_equal(ga[N0:], geno)
        # e, z (from the selected-locus table) and everything else: the host route's
        _assert_same(a, b, 'straight after the call')
        # the source was only read
        _assert_same(_columns(src, nat), src_before, 'source')

        if large:
            for d in (A, B):
                d.pop_dynamics_die(False, True)
                d.step_index = d.step_index + 1
            assert A.counts() == B.counts()
        for c, T in enumerate((3, 5)):
            for d in (A, B):
                d.walk(T, False, True)
            ha = [tuple(int(v) for v in r) for r in zip(*A.walk_history())]
            hb = [tuple(int(v) for v in r) for r in zip(*B.walk_history())]
            assert ha == hb and len(ha) == T, (c, ha, hb)
            a = _columns(A, nat)
            _assert_same(a, _columns(B, nat), 'after walk(%d)' % T)
            np.testing.assert_array_equal(_genomes(A, nat), _genomes(B, nat))
            if c == 0:
                ids = np.concatenate([rng.choice(a['ids'][a['ids'] < FIRST_ID], 3, replace=False),
                                      rng.choice(a['ids'][a['ids'] >= FIRST_ID], 5, replace=False)])
                loci = rng.randint(1, PP_L, ids.size).astype(np.int32)
                homs = rng.randint(0, 2, ids.size).astype(np.uint8)
                for d in (A, B):
                    d.mutate(_slots_of(d, nat, ids), loci, homs)
        assert (a['ids'] >= FIRST_ID + n).sum() > 50      # offspring born since the call
        _halves(A)
        _halves(B)
        np.testing.assert_array_equal(_genomes(A, nat), _genomes(B, nat))
    finally:
        A.close()
        B.close()
        if own_src is not None:
            own_src[0].close()


# ------------------------------------------------------------------ 2. fitness
def test_newcomers_fitness_is_the_death_kernels(source):
    """`fit` of the newcomers = max(prod_t (1 - phi_t |e^(not univ_adv) - z_t|^gamma_t), 0.001) x
    prod_del (1 - s_l (g_l0 + g_l1)) (csrc/gnx_kernels_demog.hip: death_prob_one), evaluated in
    float64 from the downloaded e, z and genomes: two traits (gamma 1 with a phi raster; gamma 2,
    universally advantageous), three deleterious loci.  The earlier individuals' fit stays."""
    src, nat = source
    rng = np.random.RandomState(3)
    rasts = np.stack([np.full((PP_H, PP_W), 0.8),
                      np.tile(np.linspace(0, 1, PP_W), (PP_H, 1))]).astype(np.float32)
    dev = nat.Device(PP_W, PP_H, 2, L=PP_L, n_traits=2, cap_inds=4096, cap_rows=4096, seed=41)
    try:
        dev.upload_rasters(rasts)
        dev.set_species_params(nat.default_species_params(mating_radius=3.0))
        loci = np.sort(rng.choice(PP_L, 30, replace=False))
        phi0 = (0.2 + 0.6 * rng.rand(PP_H, PP_W)).astype(np.float32)
        dev.set_trait(0, loci[:12], 0.08 * np.where(np.arange(12) % 2, -1.0, 1.0), 1, phi0, 1.0, False)
        dev.set_trait(1, loci[12:27], np.full(15, 0.03), 0, 0.9, 2.0, True)
        dloci, ds = loci[27:], np.array([0.05, 0.2, 0.35])
        dev.set_deleterious(dloci, ds)
        dev.set_recomb_paths(_paths(False))
        N0 = 200
        dev.upload_population(rng.rand(N0) * PP_W, rng.rand(N0) * PP_H, np.zeros(N0), np.zeros(N0),
                              np.arange(N0))
        g = rng.randint(0, 2 ** 63, (N0, 2, dev.W64), dtype=np.int64).astype(np.uint64)
        g[:, :, PP_L // 64] &= np.uint64((1 << (PP_L % 64)) - 1)
        g[:, :, PP_L // 64 + 1:] = 0
        dev.upload_genomes(g)
        fit_before = dev.download(nat.F_FIT).copy()
        n = 1200
        slots = rng.choice(src.N, n, replace=False)
        x, y = _coords(rng, n)
        dev.transplant(src, slots, x, y, FIRST_ID)
        e = dev.download(nat.F_E).astype(np.float64)[:, N0:]
        z = dev.download(nat.F_Z).astype(np.float64)[:, N0:]
        fit = dev.download(nat.F_FIT)
        np.testing.assert_array_equal(fit[:N0], fit_before)
        cx, cy = x.astype(np.int64), y.astype(np.int64)
        w = (1.0 - phi0.astype(np.float64)[cy, cx] * np.abs(e[1] - z[0])) * \
            (1.0 - 0.9 * np.abs(1.0 - z[1]) ** 2.0)
        w = np.maximum(w, 0.001)
        geno = dev.download_genomes(np.arange(N0, N0 + n))
        for l, s in zip(dloci, ds):
            cnt = ((geno[:, :, l >> 6] >> np.uint64(l & 63)) & np.uint64(1)).sum(axis=1)
            w = w * (1.0 - cnt.astype(np.float64) * s)
        assert w.min() < 0.5 < w.max()                # the terms matter
        rel = np.abs(fit[N0:].astype(np.float64) - w) / w
        print('fitness: max relative difference %.3g (bar %.1g)' % (rel.max(), FIT_RTOL))
        assert rel.max() <= FIT_RTOL
    finally:
        dev.close()


# ------------------------------------------------------------------ 3. / 4. sharing and GNX_OWN
def _take_everybody(source, rng):
    src, nat = source
    A, _ = _make(_paths(False), seed=29, cap_inds=8192, cap_rows=4096)
    hs = _halves(src)
    n = src.N
    # the fixture must have sharing to keep: a source whose blocks are (nearly) all its own
    # would let this test pass without showing anything
    assert hs['rows'] == PP_NB * n
    assert hs['used'] <= 0.7 * 2 * PP_NB * n, 'no sharing in the source: %r' % (hs,)
    before = _halves(A)
    x, y = _coords(rng, n)
    out = A.transplant(src, np.arange(n), x, y, FIRST_ID)
    return A, hs, before, out


def test_sharing_survives(source):
    src, nat = source
    A, hs, before, out = _take_everybody(source, np.random.RandomState(1))
    try:
        after = _halves(A)
        print('source: %d logical blocks, %d physical; recipient grew by %d' % (
            2 * hs['rows'], hs['used'], after['used'] - before['used']))
        assert after['used'] - before['used'] == hs['used']
        assert out['blocks_copied'] == hs['used']
        assert out['blocks_linked'] == 2 * hs['rows']
        assert after['rows'] - before['rows'] == hs['rows']
        np.testing.assert_array_equal(A.download_genomes(np.arange(out['first_slot'], A.N)),
                                      src.download(nat.F_GENO))
    finally:
        A.close()


def test_shared_blocks_are_not_mutated_in_place(source):
    """20 mutations of random newcomers: exactly those bits change in the recipient - a block
    two newcomers share is copied first (no GNX_OWN), or a relative would mutate too - and
    nothing changes in the source"""
    src, nat = source
    rng = np.random.RandomState(2)
    A, hs, before, out = _take_everybody(source, rng)
    try:
        g0 = A.download(nat.F_GENO)
        s0 = src.download(nat.F_GENO)
        slots = rng.randint(out['first_slot'], A.N, 20).astype(np.int64)
        loci = rng.randint(0, PP_L, 20).astype(np.int32)
        homs = rng.randint(0, 2, 20).astype(np.uint8)
        A.mutate(slots, loci, homs)
        exp = g0.copy()
        for s, l, hh in zip(slots, loci, homs):
            exp[s, hh, l >> 6] |= np.uint64(1) << np.uint64(l & 63)
        assert (exp != g0).sum() >= 5                  # (most of the 20 hit a 0 allele)
        g1 = A.download(nat.F_GENO)
        bad = np.nonzero((g1 != exp).any(axis=(1, 2)))[0]
        assert bad.size == 0, 'genomes other than expected after the mutations: slots %s' % bad[:10]
        np.testing.assert_array_equal(src.download(nat.F_GENO), s0)
        _halves(A)
    finally:
        A.close()


# ------------------------------------------------------------------ 5. capacity
def test_too_few_rows_is_code_2_and_changes_nothing(source):
    src, nat = source
    A, _ = _make(_paths(False), seed=29, cap_inds=4096, cap_rows=1900)
    try:
        A.walk(3, False, True)
        free_rows = A.genome_info()['free_rows']
        n = free_rows + 1
        assert 0 < n <= src.N and A.N + n <= 4096      # (slots would fit: the rows do not)
        rng = np.random.RandomState(4)
        x, y = _coords(rng, n)
        before, gb, hb = _columns(A, nat), _genomes(A, nat), _halves(A)
        sb, sgb = _columns(src, nat), _genomes(src, nat)
        with pytest.raises(nat.GnxError, match='capacity exceeded') as ei:
            A.transplant(src, rng.choice(src.N, n, replace=False), x, y, FIRST_ID)
        assert ei.value.code == 2
        assert A.N == before['ids'].size and A.genome_info()['free_rows'] == free_rows
        _assert_same(_columns(A, nat), before, 'recipient after the refusal')
        np.testing.assert_array_equal(_genomes(A, nat), gb)
        assert _halves(A) == hb
        _assert_same(_columns(src, nat), sb, 'source after the refusal')
        np.testing.assert_array_equal(_genomes(src, nat), sgb)
        # one fewer fits, and the handle goes on
        out = A.transplant(src, np.arange(n - 1), x[:n - 1], y[:n - 1], FIRST_ID)
        assert A.N == before['ids'].size + n - 1 and A.genome_info()['free_rows'] == 0
        _halves(A)
    finally:
        A.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals(source):
    src, nat = source
    A, _ = _make(_paths(False), seed=29)
    other_L = nat.Device(PP_W, PP_H, 2, L=6400, n_traits=0, cap_inds=1024, cap_rows=1024, seed=1)
    try:
        N0 = A.N
        max_alive = int(A.download(nat.F_ID).max())
        x = np.float32([1.5, 2.5, 3.5])
        y = np.float32([4.5, 5.5, 6.5])
        ok = np.array([0, 1, 2])
        cases = [
            ('same handle', lambda: src.transplant(src, ok, x, y, FIRST_ID)),
            ('different lengths', lambda: other_L.transplant(src, ok, x, y, FIRST_ID)),
            ('different lengths', lambda: A.transplant(other_L, ok, x, y, FIRST_ID)),
            ('not above the recipient', lambda: A.transplant(src, ok, x, y, max_alive)),
            ('off the recipient', lambda: A.transplant(src, ok, np.float32([1.5, PP_W, 3.5]), y, FIRST_ID)),
            ('off the recipient', lambda: A.transplant(src, ok, x, np.float32([-0.5, 1, 1]), FIRST_ID)),
            ('listed twice', lambda: A.transplant(src, [5, 9, 5], x, y, FIRST_ID)),
            ('slot out of range', lambda: A.transplant(src, [0, 1, src.N], x, y, FIRST_ID)),
            ('slot out of range', lambda: A.transplant(src, [0, -1, 2], x, y, FIRST_ID)),
        ]
        for match, call in cases:
            with pytest.raises(nat.GnxError, match=match) as ei:
                call()
            assert ei.value.code == 1
            assert A.N == N0
        with pytest.raises(ValueError):
            A.transplant(src, ok, x[:2], y, FIRST_ID)
        # nobody to move is no error, and the handle still takes newcomers afterwards
        assert A.transplant(src, [], [], [], FIRST_ID)['first_slot'] == N0 and A.N == N0
        A.transplant(src, ok, x, y, FIRST_ID)
        assert A.N == N0 + 3
    finally:
        A.close()
        other_L.close()


# ------------------------------------------------------------------ 7. the Model API
def _models(source_K_factor=0.5):
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    mod = gnx.make_model(small_params(seed=3))
    ps = small_params(seed=4)
    ps['comm']['species']['spp_0']['init']['K_factor'] = source_K_factor
    src = gnx.make_model(ps)
    for m, T in ((mod, 3), (src, 8)):
        m.walk(10000, 'burn', verbose=False)
        m.walk(T, 'main', verbose=False)
    return mod, src


def _api_scenario(n, source_K_factor=0.5):
    """burn both models in, add `n` of the source's individuals, then three listed ones"""
    mod, src = _models(source_K_factor)
    spp, sspp = mod.comm[0], src.comm[0]
    src_ids = np.array([*sspp])
    assert src_ids.size > n + 3
    n0, max0, Nt0, cap0 = len(spp), spp.max_ind_idx, list(spp.Nt), spp._cap
    nb0, nd0 = list(spp.n_births), list(spp.n_deaths)
    with pytest.warns(UserWarning):
        mod.add_individuals(n, (12.5, 7.25), recip_spp=0, source_spp=sspp)
    assert len(spp) == n0 + n and spp.max_ind_idx == max0 + n
    new = np.arange(max0 + 1, max0 + n + 1)
    np.testing.assert_array_equal(np.array([*spp])[-n:], new)
    np.testing.assert_array_equal(mod.get_coords(individs=new), np.float32([[12.5, 7.25]] * n))
    chosen = src_ids[:n]                                   # the n smallest ids of the source
    np.testing.assert_array_equal(mod.get_genotypes(individs=new, biallelic=True),
                                  src.get_genotypes(individs=chosen, biallelic=True))
    np.testing.assert_array_equal(spp._get_age(individs=new), sspp._get_age(individs=chosen))
    np.testing.assert_array_equal(spp._get_sex(individs=new), sspp._get_sex(individs=chosen))
    # fitness is right straight after the call (reference structs/species.py:2069-2072)
    w = np.clip(mod.get_fitness(trt=0, individs=new) * mod.get_fitness(trt=1, individs=new),
                0.001, None)
    np.testing.assert_allclose(mod.get_fitness(individs=new), w, rtol=2e-5)
    # the `individs` form: taken in ascending id order whatever order they are listed in
    pick = src_ids[[n + 2, 5, n]]
    xy = np.array([[1.0, 2.0], [3.0, 4.0], [29.999, 29.999]])     # (the border is inclusive)
    with pytest.warns(UserWarning):
        mod.add_individuals(None, xy, recip_spp='spp_0', source_spp=sspp, individs=pick)
    new2 = np.arange(max0 + n + 1, max0 + n + 4)
    assert len(spp) == n0 + n + 3 and spp.max_ind_idx == max0 + n + 3
    np.testing.assert_array_equal(np.array([*spp])[-3:], new2)
    np.testing.assert_array_equal(mod.get_coords(individs=new2), np.float32(xy))
    np.testing.assert_array_equal(mod.get_genotypes(individs=new2, biallelic=True),
                                  src.get_genotypes(individs=np.sort(pick), biallelic=True))
    assert spp.Nt == Nt0 and spp.n_births == nb0 and spp.n_deaths == nd0
    assert len(sspp) == src_ids.size                       # the source keeps its individuals
    # (not `fit`: a grown device state starts the earlier individuals' at 0 until their next step)
    state = dict(ids=np.array([*spp]), xy=mod.get_coords(), g=mod.get_genotypes(biallelic=True),
                 age=spp._get_age(), z=mod.get_z())
    mod.walk(5, 'main', verbose=False)
    assert spp.Nt[-1] == len(spp) and len(spp.Nt) == len(Nt0) + 5
    state['Nt'] = np.array(spp.Nt)
    state['ids_after'] = np.array([*spp])
    return state, spp._cap > cap0


def test_model_add_individuals():
    state, grew = _api_scenario(50)
    assert not grew


def test_model_add_individuals_grows_the_device(monkeypatch):
    """GNX_CAP_FACTOR so low that the newcomers do not fit: the recipient moves to a larger
    device state and the call gives what it gives with room to spare"""
    n = 1000
    ref, grew = _api_scenario(n, source_K_factor=2.0)
    assert not grew
    monkeypatch.setenv('GNX_CAP_FACTOR', '0.5')
    got, grew = _api_scenario(n, source_K_factor=2.0)
    assert grew
    _assert_same(got, ref, 'grown device')


def test_model_add_individuals_refusals(monkeypatch):
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    mod, src = _models()
    spp, sspp = mod.comm[0], src.comm[0]
    n0 = len(spp)
    with pytest.warns(UserWarning):
        with pytest.raises(NotImplementedError, match='msprime'):
            mod.add_individuals(5, (1, 1), source_msprime_params={'recomb_rate': 0.5,
                                                                  'mut_rate': 0.0})
        for which in (spp, sspp):
            with monkeypatch.context() as mp:
                mp.setattr(which, '_tt', object())
                with pytest.raises(NotImplementedError, match='pedigree'):
                    mod.add_individuals(5, (1, 1), source_spp=sspp)
            with monkeypatch.context() as mp:
                mp.setattr(which, '_comm', object(), raising=False)
                with pytest.raises(NotImplementedError, match='tiled'):
                    mod.add_individuals(5, (1, 1), source_spp=sspp)
        with pytest.raises(AssertionError, match='exactly one'):
            mod.add_individuals(5, (1, 1))
        with pytest.raises(AssertionError, match='exactly one'):
            mod.add_individuals(5, (1, 1), source_spp=sspp, source_msprime_params={})
        with pytest.raises(AssertionError, match="exactly one of 'n' and 'individs'"):
            mod.add_individuals(5, (1, 1), source_spp=sspp, individs=[*sspp][:5])
        with pytest.raises(AssertionError, match='Landscape'):
            mod.add_individuals(5, (30.0, 1), source_spp=sspp)
        with pytest.raises(AssertionError, match='Species object'):
            mod.add_individuals(5, (1, 1), source_spp=3.5)
        fresh = gnx.make_model(small_params(seed=5))
        with pytest.raises(AssertionError, match='burned in'):
            fresh.add_individuals(5, (1, 1), source_spp=sspp)
    assert len(spp) == n0 and len(fresh.comm[0]) == 300
