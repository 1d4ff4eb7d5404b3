"""Genetic PCA of a population from products with its dosage matrix (reference
sim/model.py:2031-2041, plot_genetic_PCA: sklearn's PCA of the speciome of mean genotypes,
ids ascending - structs/species.py:1386-1436).

D is the n x L matrix of dosages d = a + b in {0, 1, 2}; the mean genotypes are X = D / 2.
Nothing here densifies D: the exact method needs only the Gram matrix D D^T
(gnx_geno_gram), the randomized one only the products D M and D^T Y (gnx_geno_matmul,
gnx_geno_rmatmul), passed in as callables so that the CPU tests can hand in numpy ones.
Sign convention (sklearn's svd_flip(u_based_decision=False)): in every component the loading
entry of largest |value| is positive.  Pure functions; torch is used only when the products
run on the device, and is imported there.
"""
import numpy as np

MAX_K = 64          # columns per device product (gnx_geno_matmul / gnx_geno_rmatmul)


def check_n_pcs(n_pcs, n, n_loci, oversample=0):
    """ValueError unless 1 <= n_pcs <= min(n - 1, n_loci, 64 - oversample)"""
    hi = min(n - 1, n_loci, MAX_K - oversample)
    if isinstance(n_pcs, bool) or int(n_pcs) != n_pcs or not 1 <= n_pcs <= hi:
        raise ValueError('n_pcs must be an integer in 1..%d (n = %d individuals, %d loci, '
                         'oversample %d); got %r' % (max(hi, 0), n, n_loci, oversample, n_pcs))
    return int(n_pcs)


def _to_numpy(a):
    if hasattr(a, 'detach'):
        return a.detach().cpu().numpy()
    return np.asarray(a)


def _signs(loadings):
    """+1 / -1 per component (rows): its entry of largest |value| becomes positive"""
    loadings = np.asarray(loadings, np.float64)
    idx = np.argmax(np.abs(loadings), axis=1)
    s = np.sign(loadings[np.arange(loadings.shape[0]), idx])
    s[s == 0] = 1.0
    return s


def pca_from_gram(G, n_pcs, rmatmul=None):
    """Exact PCA of a sample from its dosage Gram matrix G = D D^T (n x n), in fp64.

    The Gram of the mean genotypes (G / 4) is double-centred (K = H G/4 H), eigh(K) gives
    K = U diag(lam) U^T; scores = U sqrt(lam) (sklearn's fit_transform, U S), ratio =
    lam / trace(K) (sklearn's explained_variance_ratio_).  rmatmul(U) = D^T U ([n][k] ->
    [L][k]) supplies the loadings (D^T u is X_c^T u up to a positive factor, u being
    orthogonal to the ones) whose largest entry fixes each component's sign; without it the
    score entry of largest |value| is made positive instead.
    -> scores [n][n_pcs], explained_variance_ratio [n_pcs]"""
    G = np.asarray(G)
    if G.ndim != 2 or G.shape[0] != G.shape[1]:
        raise ValueError('G must be square, got shape %s' % (G.shape,))
    n = G.shape[0]
    n_pcs = check_n_pcs(n_pcs, n, n)
    K = G.astype(np.float64) / 4.0
    r = K.mean(axis=1)
    K = K - r[:, None] - r[None, :] + r.mean()
    lam, U = np.linalg.eigh(K)
    lam = np.maximum(lam[::-1][:n_pcs], 0.0)
    U = np.ascontiguousarray(U[:, ::-1][:, :n_pcs])
    scores = U * np.sqrt(lam)
    ratio = lam / np.trace(K)
    s = _signs(_to_numpy(rmatmul(U)).T if rmatmul is not None else U.T)
    return scores * s, ratio


class _Numpy:
    """numpy products: the callables get fp64 as it is"""
    f64 = staticmethod(lambda a: np.asarray(a, np.float64))
    arg = staticmethod(lambda a: a)
    qr = staticmethod(lambda a: np.linalg.qr(a)[0])
    put = staticmethod(lambda a: np.asarray(a, np.float64))
    colsum = staticmethod(lambda a: a.sum(0, keepdims=True))


class _Torch:
    """device products: their inputs go in fp32, everything between them is fp64 there"""

    def __init__(self, like):
        import torch
        self.torch = torch
        self.dev = like.device

    def f64(self, a):
        return a.to(self.torch.float64)

    def arg(self, a):
        return a.to(self.torch.float32).contiguous()

    def qr(self, a):
        return self.torch.linalg.qr(a)[0]

    def put(self, a):
        return self.torch.as_tensor(np.asarray(a, np.float64), device=self.dev)

    def colsum(self, a):
        return a.sum(0, keepdim=True)


def randomized_pca(matmul, rmatmul, mu, n, L, n_pcs, oversample=10, n_iter=8, seed=0,
                   sumsq=None):
    """Halko-Martinsson-Tropp subspace iteration on the centred mean genotypes
    X_c = (D - 1 mu^T) / 2, the centring applied algebraically:
        X_c M   = (D M - 1 (mu^T M)) / 2,    X_c^T Y = (D^T Y - mu (1^T Y)) / 2.
    matmul(M [L][l]) -> D M [n][l] and rmatmul(Y [n][l]) -> D^T Y [L][l], l = n_pcs +
    oversample.  mu: per-locus mean dosage [L]; a torch tensor puts the iteration on its
    device (products fed fp32, QR re-orthonormalisation in fp64 after every product), a
    numpy array keeps it in numpy.  sumsq: per-locus sum of squared dosages [L] (cnt1 +
    2 hom11 from the locus counts): the exact total variance of the ratio.  The starting
    block is numpy RandomState(seed).standard_normal((L, l)).
    -> scores [n][n_pcs], explained_variance_ratio [n_pcs] (numpy fp64)"""
    n, L = int(n), int(L)
    if int(oversample) != oversample or oversample < 0:
        raise ValueError('oversample must be a non-negative integer')
    if int(n_iter) != n_iter or n_iter < 0:
        raise ValueError('n_iter must be a non-negative integer')
    n_pcs = check_n_pcs(n_pcs, n, L, oversample)
    if sumsq is None:
        raise ValueError('sumsq (per-locus sum of squared dosages) is required for the ratio')
    l = n_pcs + int(oversample)
    mu_np = _to_numpy(mu).astype(np.float64).reshape(L)
    xp = _Torch(mu) if hasattr(mu, 'detach') else _Numpy()
    mu_c = xp.put(mu_np.reshape(L, 1))

    def A(M):            # X_c M
        return (xp.f64(matmul(xp.arg(M))) - mu_c.T @ M) * 0.5

    def At(Y):           # X_c^T Y
        return (xp.f64(rmatmul(xp.arg(Y))) - mu_c @ xp.colsum(Y)) * 0.5

    Q = xp.qr(A(xp.put(np.random.RandomState(seed).standard_normal((L, l)))))
    for _ in range(int(n_iter)):
        Q = xp.qr(A(xp.qr(At(Q))))
    Bt = _to_numpy(At(Q))                               # (Q^T X_c)^T, L x l
    Ub, s, Vt = np.linalg.svd(Bt.T, full_matrices=False)
    scores = _to_numpy(Q) @ (Ub[:, :n_pcs] * s[:n_pcs])
    total = float((np.asarray(sumsq, np.float64) - n * mu_np ** 2).sum()) / 4.0
    return scores * _signs(Vt[:n_pcs]), s[:n_pcs] ** 2 / total


def device_randomized_pca(dev, n_pcs, loci=None, oversample=10, n_iter=8, seed=0):
    """randomized_pca of the whole living population of a Device (slot order), on the
    device: products gnx_geno_matmul / gnx_geno_rmatmul, mean and total variance from
    gnx_stats_locus_counts; loci restricts the columns (M is zero elsewhere)."""
    import torch
    n, L = int(dev.N), int(dev.L)
    cnt1, het = dev.stats_locus_counts()
    cnt1 = cnt1.astype(np.float64)
    sumsq = cnt1 + (cnt1 - het)          # sum d^2 = cnt1 + 2 hom11, hom11 = (cnt1 - cnt_het) / 2
    tdev = torch.device('cuda', int(dev.cfg.device))
    if loci is None:
        mu = torch.as_tensor(cnt1 / max(n, 1), device=tdev)
        return randomized_pca(dev.geno_matmul, dev.geno_rmatmul, mu, n, L, n_pcs,
                              oversample=oversample, n_iter=n_iter, seed=seed, sumsq=sumsq)
    loci_np = np.asarray(loci, np.int64)
    loci_t = torch.as_tensor(loci_np, device=tdev)

    def matmul(M):
        full = torch.zeros((L, M.shape[1]), dtype=torch.float32, device=tdev)
        full[loci_t] = M
        return dev.geno_matmul(full)

    def rmatmul(Y):
        return dev.geno_rmatmul(Y)[loci_t]

    mu = torch.as_tensor(cnt1[loci_np] / max(n, 1), device=tdev)
    return randomized_pca(matmul, rmatmul, mu, n, loci_np.size, n_pcs, oversample=oversample,
                          n_iter=n_iter, seed=seed, sumsq=sumsq[loci_np])
