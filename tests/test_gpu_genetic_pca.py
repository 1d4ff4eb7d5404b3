"""Genetic PCA and genetic distances on the device (csrc/gnx_geno.hip, sim/pca.py,
Species._calc_genetic_PCA / _calc_genetic_distances) against numpy / torch-fp64 products of the
downloaded genomes and against the exact SVD.  Needs an MI355X.

Exactness: Gram matrices are int64-equal; products with integer inputs whose absolute sums stay
below 2^24 are equal to the exact product; with standard-normal inputs every output is within
n_terms 2^-23 (|D| |M|) of the exact product (n_terms = loci or individuals summed: twice the
worst-case bound of an fp32 sum of exact products in any order).  The oracle's products run in
fp64 on the GPU (torch): integer entries below 2^53 make them exact."""
import numpy as np
import pytest

from test_gpu_parity import native
from test_gpu_product_path import _make, _paths, L as PP_L
from test_genetic_pca_host import planted, reference_pca, assert_gaps, max_sine

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23


def _dosages(packed, L):
    """dosages float64 [n][L] on the GPU of packed genomes uint64 [n][2][W64]"""
    import torch
    sh = torch.arange(64, device='cuda', dtype=torch.int64)
    out = []
    for r0 in range(0, packed.shape[0], 256):
        t = torch.from_numpy(np.ascontiguousarray(packed[r0:r0 + 256]).view(np.int64)).cuda()
        b = ((t.unsqueeze(-1) >> sh) & 1).reshape(t.shape[0], 2, -1)[:, :, :L]
        out.append((b[:, 0] + b[:, 1]).to(torch.float64))
    return torch.cat(out)


def _mask(loci, W64):
    m = np.zeros(W64, np.uint64)
    np.bitwise_or.at(m, loci >> 6, np.uint64(1) << (loci & 63).astype(np.uint64))
    return m


@pytest.fixture(scope='module')
def walked():
    """the product path: a 2^20-slot handle (lazy mortality between the steps of a walk, the
    crossover launched behind the next step, blocks shared with parents) walked in pieces with
    a mutation and a forced collection between them; about 12 000 alive"""
    nat = native()
    dev, _ = _make(_paths(False), cap_inds=1 << 20, cap_rows=1 << 15, N=12000, K_factor=8.0)
    rng = np.random.RandomState(5)
    for c, T in enumerate((4, 3, 5)):
        dev.walk(T, False, True)
        if c == 0:
            slots = rng.choice(dev.N, 6, replace=False)
            dev.mutate(slots, rng.randint(1, PP_L, 6).astype(np.int32),
                       rng.randint(0, 2, 6).astype(np.uint8))
        if c == 1:
            rows, broken, _, used, free, total = (int(v) for v in dev.debug_halves())
            assert broken == 0 and used + free == total
    pc = dev.path_counts()
    assert pc['lazy_mortalities'] > 0 and pc['xo_launch_p2'] > 0, pc
    assert dev.N > 8192, dev.N
    yield dev, nat
    dev.close()


@pytest.mark.parametrize('masked', [False, True], ids=['all_loci', 'mask'])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 8192])
def test_gram_exact_on_product_path(walked, n, masked):
    import torch
    dev, nat = walked
    rng = np.random.RandomState(n + 7 * masked)
    slots = rng.choice(dev.N, n, replace=False).astype(np.int64)
    D = _dosages(dev.download_genomes(slots), PP_L)
    mask = None
    if masked:
        loci = np.sort(rng.choice(PP_L, 3000, replace=False))
        loci[-1] = PP_L - 1                      # the last word, next to the padding
        mask = _mask(loci, dev.W64)
        D = D[:, torch.as_tensor(loci, device='cuda')]
    G = dev.geno_gram(slots, mask)
    ref = (D @ D.T).round().to(torch.int64).cpu().numpy()
    np.testing.assert_array_equal(G, ref)
    G2 = dev.geno_gram(slots, mask)              # back to back: the same
    np.testing.assert_array_equal(G2, G)


def test_gram_limits(walked):
    dev, nat = walked
    with pytest.raises(nat.GnxError, match='8192'):
        dev.geno_gram(np.arange(8193))
    with pytest.raises(nat.GnxError, match='8192'):
        dev.geno_gram()                          # all living slots: more than 8192
    with pytest.raises(nat.GnxError, match='slot out of range'):
        dev.geno_gram(np.array([0, dev.N]))


@pytest.mark.parametrize('k', [1, 16, 17, 64])
def test_products_integer_exact_on_product_path(walked, k):
    import torch
    dev, nat = walked
    rng = np.random.RandomState(k)
    for slots in (rng.choice(dev.N, 5000, replace=False).astype(np.int64), None):
        packed = dev.download_genomes(np.arange(dev.N) if slots is None else slots)
        D = _dosages(packed, PP_L)
        n = D.shape[0]
        M = torch.as_tensor(rng.randint(-4, 5, (PP_L, k)), dtype=torch.float32, device='cuda')
        Y = dev.geno_matmul(M, slots)             # sum |D||M| <= 8 L < 2^24: exact
        assert Y.shape == (n, k)
        torch.testing.assert_close(Y.double(), D @ M.double(), rtol=0, atol=0)
        Yi = torch.as_tensor(rng.randint(-4, 5, (n, k)), dtype=torch.float32, device='cuda')
        Z = dev.geno_rmatmul(Yi, slots)           # sum |D||Y| <= 8 n < 2^24: exact
        assert Z.shape == (PP_L, k)
        torch.testing.assert_close(Z.double(), D.T @ Yi.double(), rtol=0, atol=0)
        # back to back, and a product of a product
        torch.testing.assert_close(dev.geno_matmul(M, slots), Y, rtol=0, atol=0)
        torch.testing.assert_close(dev.geno_rmatmul(Yi, slots), Z, rtol=0, atol=0)
        del D


def _plain(L, N, seed):
    """a handle with N random genomes of L loci (uploaded: rows in slot order)"""
    nat = native()
    dev = nat.Device(16, 16, 1, L=L, cap_inds=N + 64, cap_rows=N + 64, seed=seed)
    dev.upload_rasters(np.ones((1, 16, 16), np.float32))
    dev.set_species_params(nat.default_species_params())
    rng = np.random.RandomState(seed)
    dev.upload_population(rng.rand(N) * 16, rng.rand(N) * 16, np.zeros(N), np.zeros(N),
                          np.arange(N))
    g = rng.randint(0, 2 ** 63, (N, 2, dev.W64), dtype=np.int64).astype(np.uint64)
    g ^= rng.randint(0, 2, g.shape).astype(np.uint64) << np.uint64(63)
    dev.upload_genomes(g)
    return dev, nat


@pytest.mark.parametrize('L', [64, 1000])
def test_products_real_within_fp32_bound(L):
    import torch
    N, k = 3000, 16
    dev, nat = _plain(L, N, 11 + L)
    D = _dosages(dev.download_genomes(np.arange(N)), L)
    g = torch.Generator(device='cuda').manual_seed(L)
    M = torch.randn((L, k), generator=g, device='cuda', dtype=torch.float32)
    Y = dev.geno_matmul(M).double()
    Md = M.double()
    err = (Y - D @ Md).abs()
    bound = L * EPS * (D @ Md.abs())
    print('L=%d matmul: worst error / bound %.3g' % (L, (err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())
    Yn = torch.randn((N, k), generator=g, device='cuda', dtype=torch.float32)
    Z = dev.geno_rmatmul(Yn).double()
    err = (Z - D.T @ Yn.double()).abs()
    bound = N * EPS * (D.T @ Yn.double().abs())
    print('L=%d rmatmul: worst error / bound %.3g' % (L, (err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())
    # an rmatmul over 64 slots
    slots = np.random.RandomState(L).choice(N, 64, replace=False).astype(np.int64)
    Y64 = Yn[:64].contiguous()
    Z = dev.geno_rmatmul(Y64, slots).double()
    Ds = D[torch.as_tensor(slots, device='cuda')]
    err = (Z - Ds.T @ Y64.double()).abs()
    bound = 64 * EPS * (Ds.T @ Y64.double().abs())
    assert bool((err <= bound).all())
    dev.close()


def test_metric_size_products_exact():
    """N = 10^6, L = 10^5 (bench.py's c4_metric set-up): D^T 1 = cnt1 of the locus counts, and
    D e_l = the dosages at locus l of a 3000-slot sample"""
    import torch
    import bench
    cfg = bench.WORKLOADS['c4_metric']
    dev, _, _ = bench.build_device(cfg, 1, 0)
    bench.setup_genomes(dev, cfg, 1)
    N, L = dev.N, cfg['L']
    cnt1, _ = dev.stats_locus_counts()
    Z = dev.geno_rmatmul(torch.ones((N, 1), dtype=torch.float32, device='cuda'))
    np.testing.assert_array_equal(Z[:, 0].cpu().numpy(), cnt1.astype(np.float32))
    rng = np.random.RandomState(3)
    loci = np.sort(rng.choice(L, 16, replace=False))
    loci[-1] = L - 1
    M = torch.zeros((L, 16), dtype=torch.float32, device='cuda')
    M[torch.as_tensor(loci, device='cuda'), torch.arange(16, device='cuda')] = 1.0
    Y = dev.geno_matmul(M).cpu().numpy()
    slots = rng.choice(N, 3000, replace=False).astype(np.int64)
    D = _dosages(dev.download_genomes(slots), L)[:, torch.as_tensor(loci, device='cuda')]
    np.testing.assert_array_equal(Y[slots], D.cpu().numpy().astype(np.float32))
    dev.close()


def _upload_dosages(D, seed):
    """a handle whose genomes carry the dosages D [n][L] (d = 1: homologue 0)"""
    import gnx_oracle as O
    nat = native()
    n, L = D.shape
    dev = nat.Device(16, 16, 1, L=L, cap_inds=n + 64, cap_rows=n + 64, seed=seed)
    dev.upload_rasters(np.ones((1, 16, 16), np.float32))
    dev.set_species_params(nat.default_species_params())
    rng = np.random.RandomState(seed)
    dev.upload_population(rng.rand(n) * 16, rng.rand(n) * 16, np.zeros(n), np.zeros(n),
                          np.arange(n))
    g = np.stack([(D >= 1), (D == 2)], axis=2).astype(np.uint8)
    dev.upload_genomes(O.pack_genomes(g))
    return dev


@pytest.mark.parametrize('pop', [(3000, 2000, 4, 0.05, 5), (20000, 1000, 4, 0.02, 6),
                                 (4000, 4096, 3, 0.03, 7)], ids=lambda p: '%dx%d' % p[:2])
def test_randomized_pca_on_device_matches_exact_svd(pop):
    from geonomics_amd.sim import pca as P
    n, L, demes, fst, seed = pop
    n_pcs = demes - 1
    D = planted(n, L, demes, fst, seed)
    X = D / 2.0
    U, s, _ = np.linalg.svd(X - X.mean(axis=0), full_matrices=False)
    assert s[n_pcs - 1] >= 2.5 * s[n_pcs], s[:n_pcs + 1]
    dev = _upload_dosages(D, seed)
    scores, ratio = P.device_randomized_pca(dev, n_pcs, oversample=10, n_iter=8, seed=0)
    sine = max_sine(U[:, :n_pcs], scores)
    rel = np.abs(np.linalg.norm(scores, axis=0) - s[:n_pcs]) / s[:n_pcs]
    print('%s: sine %.3g, singular value error %.3g' % (pop, sine, rel.max()))
    assert sine <= 1e-5
    assert rel.max() <= 1e-6
    dev.close()


def _small_model(seed):
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    mod = gnx.make_model(small_params(seed=seed))
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(12, 'main', verbose=False)
    return mod


def test_model_genetic_pca_and_distances():
    mod = _small_model(5)
    ids = np.array([*mod.comm[0]])
    gts = mod.get_genotypes()                       # mean genotypes, ids ascending
    got_ids, dist = mod.get_genetic_distances()
    np.testing.assert_array_equal(got_ids, ids)
    ref = np.sqrt(((gts[:, None, :] - gts[None, :, :]) ** 2).sum(axis=2))
    np.testing.assert_array_equal(dist, ref)         # bit for bit
    sub = ids[::3]
    got_ids, dist = mod.get_genetic_distances(individs=sub[::-1], loci=np.arange(10, 50))
    np.testing.assert_array_equal(got_ids, sub)
    g = gts[::3, 10:50]
    np.testing.assert_array_equal(dist, np.sqrt(((g[:, None] - g[None]) ** 2).sum(axis=2)))
    n_pcs = 3
    ref_scores, ref_ratio, s = reference_pca(gts * 2.0, n_pcs)
    assert_gaps(s, n_pcs)
    got_ids, scores, ratio = mod.calc_genetic_PCA(n_pcs=n_pcs)
    np.testing.assert_array_equal(got_ids, ids)
    print('model PCA: score error %.3g s_1' % (np.abs(scores - ref_scores).max() / s[0]))
    assert np.abs(scores - ref_scores).max() <= 1e-9 * s[0]
    assert np.abs(ratio - ref_ratio).max() <= 1e-12


def test_errors():
    import geonomics_amd as gnx
    nat = native()
    dev = nat.Device(16, 16, 1, L=1000, cap_inds=256, cap_rows=256, seed=1)
    dev.upload_rasters(np.ones((1, 16, 16), np.float32))
    dev.set_species_params(nat.default_species_params())
    dev.upload_population(np.ones(10), np.ones(10), np.zeros(10), np.zeros(10), np.arange(10))
    import torch
    for call in (lambda: dev.geno_gram(),
                 lambda: dev.geno_matmul(torch.zeros((1000, 4), device='cuda')),
                 lambda: dev.geno_rmatmul(torch.zeros((10, 4), device='cuda'))):
        with pytest.raises(nat.GnxError, match='genomes not assigned'):
            call()
    dev.close()
    mod = _small_model(5)
    ids = np.array([*mod.comm[0]])
    with pytest.raises(ValueError, match='not alive'):
        mod.calc_genetic_PCA(individs=[ids[0], ids[-1] + 1000])
    with pytest.raises(ValueError, match='not alive'):
        mod.get_genetic_distances(individs=[-1])
    for bad in (0, len(ids), 55):
        with pytest.raises(ValueError, match='n_pcs'):
            mod.calc_genetic_PCA(n_pcs=bad)
    from geonomics_amd.structs.tiled import TiledSpecies
    with pytest.raises(NotImplementedError):
        TiledSpecies._calc_genetic_PCA(mod.comm[0])
    with pytest.raises(NotImplementedError):
        TiledSpecies._calc_genetic_distances(mod.comm[0])
