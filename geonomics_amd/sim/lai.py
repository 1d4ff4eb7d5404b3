"""Local ancestry: the linkage model of Falush, Stephens & Pritchard (2003) with the ancestral
allele frequencies held fixed and one admixture time, painted along every phased haplotype by
the forward-backward recurrences of a hidden Markov model (csrc/gnx_lai.hip, gnx_lai_paint).

The hidden state of haplotype t at used locus l is its ancestry z in 0..K-1.  q [K] is the prior
of the individual (both homologues share it), f[l][k] = P(allele 1 | ancestry k), g = fl(1 - f),
E_k = f[l][k] where the haplotype carries a 1 and g[l][k] where it carries a 0.  Between used
loci l - 1 and l, d_l Morgans apart, the ancestry is drawn anew from q with probability
sw_l = -expm1(-gens d_l) and kept with stay_l = fl(1 - sw_l); sw_0 = 1, stay_0 = 0.

Forward, l = 0 .. L_u - 1, alpha_{-1} = q:
    b_k = (stay_l alpha_{l-1,k} + sw_l q_k) E_k,  c = b_0 + b_1 + ...,  alpha_{l,k} = b_k / c,
    loglik += ln c
Backward, beta_{L_u-1,k} = 1, l = L_u - 1 .. 0:
    p_k = alpha_{l,k} beta_{l,k},  gamma_{l,k} = p_k / (p_0 + p_1 + ...)
    l > 0:  w_k = beta_{l,k} E_k,  u = q_0 w_0 + q_1 w_1 + ...,  b'_k = stay_l w_k + sw_l u,
            beta_{l-1,k} = b'_k / (b'_0 + b'_1 + ...)
Every sum over k runs left to right.  brute_paint restates this in numpy with the device's
operations in the device's order, so that all it returns but the log-likelihood is the device's
bit for bit; enumerate_paths sums over all K^L paths.  Pure numpy: nothing here needs the
library.
"""
import itertools
import math

import numpy as np

MAX_K = 8            # gnx_lai_paint's template instances
MAX_GROUPS = 64      # groups of anc_locus per call
EPS = 1e-3           # F lives in [EPS, 1 - EPS] unless the caller says so
# tract-length histogram of calls_to_tracts, Morgans
TRACT_EDGES = np.array([0.0, 0.001, 0.002, 0.005, 0.01, 0.02, 0.05, 0.1, 0.2, 0.5, 1.0, np.inf])


# ---------------------------------------------------------------- the inputs
def switch_probs(pos, gens):
    """(sw, stay) [L_u] from the Haldane coordinates (Morgans, non-decreasing) of the used loci
    and the generations since admixture: sw_l = -expm1(-gens (pos_l - pos_{l-1})),
    stay_l = fl(1 - sw_l), sw_0 = 1, stay_0 = 0"""
    pos = np.asarray(pos, dtype=np.float64).ravel()
    if pos.size < 1 or not np.isfinite(pos).all() or (np.diff(pos) < 0).any():
        raise ValueError('pos: a non-empty list of finite, non-decreasing map positions')
    gens = check_gens(gens)
    sw = np.ones(pos.size)
    sw[1:] = -np.expm1(-gens * np.diff(pos))
    stay = 1.0 - sw
    return sw, stay


def clip_freqs(F, eps=EPS):
    """F clipped to [eps, 1 - eps]"""
    if isinstance(eps, bool) or not 0.0 < float(eps) < 0.5:
        raise ValueError('eps: a number in (0, 0.5) (got %r)' % (eps,))
    F = np.array(F, dtype=np.float64)
    if not np.isfinite(F).all():
        raise ValueError('F: finite frequencies')
    return np.clip(F, float(eps), 1.0 - float(eps))


def check_K(K):
    if isinstance(K, bool) or int(K) != K or not 1 <= K <= MAX_K:
        raise ValueError('K: a number of ancestral populations in 1..%d (got %r)' % (MAX_K, K))
    return int(K)


def check_gens(gens):
    if isinstance(gens, (bool, str)) or not (np.isfinite(gens) and gens > 0):
        raise ValueError("gens: a positive finite number of generations, or 'fit' (got %r)"
                         % (gens,))
    return float(gens)


def check_prior(prior, n, K):
    """'uniform', or rows [n][K] >= 0 that sum to 1 -> fp64 [n][K]"""
    if isinstance(prior, str):
        if prior != 'uniform':
            raise ValueError("prior: 'fit', 'uniform' or an array (n, K) (got %r)" % (prior,))
        return np.full((n, K), 1.0 / K)
    Q = np.array(prior, dtype=np.float64)
    if Q.shape != (n, K):
        raise ValueError('prior: an array of shape %s, not (n, K) = (%d, %d)' % (Q.shape, n, K))
    if not (np.isfinite(Q).all() and (Q >= 0).all()
            and (np.abs(Q.sum(axis=1) - 1.0) <= 1e-9).all()):
        raise ValueError('prior: rows of probabilities that sum to 1')
    return Q


def check_by(by, n):
    """labels per analysed individual (-1: left out) -> (int32 [n] or None, n_groups)"""
    if by is None:
        return None, 0
    b = np.asarray(by)
    if b.shape != (n,) or not np.issubdtype(b.dtype, np.integer):
        raise ValueError('by: one integer label per analysed individual (%d of them)' % n)
    if b.min() < -1 or b.max() >= MAX_GROUPS or b.max() < 0:
        raise ValueError('by: labels in -1..%d (-1: left out), at least one of them >= 0'
                         % (MAX_GROUPS - 1))
    return b.astype(np.int32), int(b.max()) + 1


def panel_freqs(ones, n_k):
    """reference-panel frequencies from the panels' counts of 1-alleles ones [K][L_u] and their
    sizes n_k [K] (individuals): (ones + 0.5) / (2 n_k + 1) -> F [K][L_u]"""
    ones = np.asarray(ones, dtype=np.float64)
    n_k = np.asarray(n_k, dtype=np.float64).ravel()
    if ones.ndim != 2 or n_k.size != ones.shape[0] or (n_k < 1).any():
        raise ValueError('panels: every panel holds at least one individual')
    return (ones + 0.5) / (2.0 * n_k[:, None] + 1.0)


def _check_paint(X, F, sw, stay, Q):
    X = np.asarray(X)
    F = np.asarray(F, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    sw = np.asarray(sw, dtype=np.float64).ravel()
    stay = np.asarray(stay, dtype=np.float64).ravel()
    if X.ndim != 3 or X.shape[2] != 2:
        raise ValueError('X: phased bits [n][L_u][2]')
    n, L_u = X.shape[:2]
    K = check_K(F.shape[1] if F.ndim == 2 else 0)
    if F.shape != (L_u, K) or Q.shape != (n, K) or sw.shape != (L_u,) or stay.shape != (L_u,):
        raise ValueError('F %s, sw %s, stay %s and Q %s do not fit X %s'
                         % (F.shape, sw.shape, stay.shape, Q.shape, X.shape))
    return X, F, sw, stay, Q, n, L_u, K


# ---------------------------------------------------------------- the call, restated
def brute_paint(X, F, sw, stay, Q, by=None, n_groups=0, want_gamma=False):
    """gnx_lai_paint restated (include/gnx_hip.h): X [n][L_u][2] the phased bits at the used
    loci, F [L_u][K], sw and stay [L_u], Q [n][K], by int [n] labels in -1..n_groups-1 or None.
    The recurrences of the module's docstring with explicit left-to-right loops over k, one
    IEEE operation at a time, vectorised over the haplotypes t = 2 i + homologue only
    -> dict(loglik [2n] (math.fsum of the ln c), loglik_abs [2n] (the fsum of |ln c|, for error
    bounds), anc_hap [2n][K] (gamma summed in descending l), anc_locus [max(n_groups, 1)][L_u][K]
    (gamma summed over the haplotypes of the group in ascending t), switches int32 [2n], calls
    uint8 [2n][L_u], gamma [2n][L_u][K] if want_gamma)"""
    X, F, sw, stay, Q, n, L_u, K = _check_paint(X, F, sw, stay, Q)
    T = 2 * n
    bits = X.transpose(1, 0, 2).reshape(L_u, T) != 0          # [l][t]
    G = 1.0 - F
    q = [np.repeat(Q[:, k], 2) for k in range(K)]
    ks = range(K)

    def emit(l):
        return [np.where(bits[l], F[l, k], G[l, k]) for k in ks]

    alpha = np.empty((L_u, K, T))
    logc = np.empty((L_u, T))
    a = list(q)
    for l in range(L_u):
        E = emit(l)
        b = [(stay[l] * a[k] + sw[l] * q[k]) * E[k] for k in ks]
        c = b[0]
        for k in range(1, K):
            c = c + b[k]
        a = [b[k] / c for k in ks]
        for k in ks:
            alpha[l, k] = a[k]
        logc[l] = np.log(c)
    cols = logc.T.tolist()
    loglik = np.array([math.fsum(r) for r in cols])
    loglik_abs = np.array([math.fsum(map(abs, r)) for r in cols])

    gamma = np.empty((T, L_u, K))
    anc_hap = np.zeros((T, K))
    calls = np.zeros((T, L_u), np.uint8)
    beta = [np.ones(T) for _ in ks]
    for l in range(L_u - 1, -1, -1):
        p = [alpha[l, k] * beta[k] for k in ks]
        s = p[0]
        for k in range(1, K):
            s = s + p[k]
        g = [p[k] / s for k in ks]
        best, call = g[0], np.zeros(T, np.uint8)
        for k in ks:
            gamma[:, l, k] = g[k]
            anc_hap[:, k] = anc_hap[:, k] + g[k]
            if k:
                up = g[k] > best
                best = np.where(up, g[k], best)
                call[up] = k
        calls[:, l] = call
        if l > 0:
            E = emit(l)
            w = [beta[k] * E[k] for k in ks]
            u = q[0] * w[0]
            for k in range(1, K):
                u = u + q[k] * w[k]
            bn = [stay[l] * w[k] + sw[l] * u for k in ks]
            s = bn[0]
            for k in range(1, K):
                s = s + bn[k]
            beta = [bn[k] / s for k in ks]
    switches = (calls[:, 1:] != calls[:, :-1]).sum(axis=1).astype(np.int32)

    lab = np.zeros(n, np.int64) if by is None else np.asarray(by, dtype=np.int64).ravel()
    n_g = max(int(n_groups), 1)
    if lab.shape != (n,) or lab.min() < -1 or lab.max() >= n_g:
        raise ValueError('by: %d labels in -1..%d' % (n, n_g - 1))
    anc_locus = np.zeros((n_g, L_u, K))
    for t in range(T):
        gi = lab[t >> 1]
        if gi >= 0:
            anc_locus[gi] = anc_locus[gi] + gamma[t]
    out = dict(loglik=loglik, loglik_abs=loglik_abs, anc_hap=anc_hap, anc_locus=anc_locus,
               switches=switches, calls=calls)
    if want_gamma:
        out['gamma'] = gamma
    return out


def enumerate_paths(x, F, sw, stay, q):
    """the model summed over all K^L ancestry paths of one haplotype x [L] (bits): the path
    z has probability prod_l (stay_l [z_l = z_{l-1}] + sw_l q[z_l]) E_{z_l}(x_l), with
    z_{-1} free under stay_0 = 0 -> (gamma [L][K], loglik)"""
    x = np.asarray(x).ravel() != 0
    F = np.asarray(F, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64).ravel()
    L, K = F.shape
    E = np.where(x[:, None], F, 1.0 - F)
    total = 0.0
    post = np.zeros((L, K))
    for z in itertools.product(range(K), repeat=L):
        p = q[z[0]] * sw[0] * E[0, z[0]]
        for l in range(1, L):
            p *= (stay[l] * (z[l] == z[l - 1]) + sw[l] * q[z[l]]) * E[l, z[l]]
        total += p
        post[np.arange(L), list(z)] += p
    return post / total, math.log(total)


# ---------------------------------------------------------------- the admixture time
def fit_gens(loglik_of_gens, lo=1.0, hi=1000.0, tol=0.01):
    """the generations since admixture of the largest total log-likelihood, by golden-section
    search on ln(gens) over [lo, hi] until the bracket is narrower than tol (in ln gens)
    -> (gens, trace [(gens, loglik)] of every evaluation, in order)"""
    if not (0.0 < lo < hi and np.isfinite(hi)):
        raise ValueError('fit_gens: 0 < lo < hi (got %r, %r)' % (lo, hi))
    if not tol > 0:
        raise ValueError('fit_gens: tol: a positive width in ln(gens) (got %r)' % (tol,))
    trace = []

    def f(x):
        g = math.exp(x)
        v = float(loglik_of_gens(g))
        trace.append((g, v))
        return v

    r = (math.sqrt(5.0) - 1.0) / 2.0
    a, b = math.log(lo), math.log(hi)
    x1, x2 = b - r * (b - a), a + r * (b - a)
    f1, f2 = f(x1), f(x2)
    while b - a > tol:
        if f1 < f2:
            a, x1, f1 = x1, x2, f2
            x2 = a + r * (b - a)
            f2 = f(x2)
        else:
            b, x2, f2 = x2, x1, f1
            x1 = b - r * (b - a)
            f1 = f(x1)
    best = max(trace, key=lambda gv: gv[1])
    return best[0], trace


# ---------------------------------------------------------------- tracts of the hard calls
def calls_to_tracts(calls, pos, brk=None, edges=None, K=None):
    """the runs of equal hard calls: calls uint8 [T][L_u], pos [L_u] the map positions of the
    used loci (Morgans), brk bool [L_u] (True: a chromosome break before locus l, which ends
    every run; None: none).  A tract's length is pos[end] - pos[start].  edges: the bounds of
    the histogram (None: TRACT_EDGES)
    -> dict(tracts: per haplotype an int64 array [m][3] of (start, end, ancestry) over used-locus
    indices, end inclusive; lengths: per haplotype fp64 [m]; hist: dict(edges, counts [K][bins],
    sum_len [K][bins]))"""
    calls = np.asarray(calls)
    pos = np.asarray(pos, dtype=np.float64).ravel()
    if calls.ndim != 2 or calls.shape[1] != pos.size or pos.size < 1:
        raise ValueError('calls [T][L_u] and pos [L_u] do not fit')
    L_u = pos.size
    cut = np.zeros(L_u, bool) if brk is None else np.asarray(brk, dtype=bool).ravel().copy()
    if cut.shape != (L_u,):
        raise ValueError('brk: one flag per used locus')
    cut[0] = True
    edges = TRACT_EDGES if edges is None else np.asarray(edges, dtype=np.float64).ravel()
    if edges.size < 2 or (np.diff(edges) <= 0).any():
        raise ValueError('edges: at least two ascending lengths')
    K = int(calls.max()) + 1 if K is None else int(K)
    counts = np.zeros((K, edges.size - 1), np.int64)
    sums = np.zeros((K, edges.size - 1))
    tracts, lengths = [], []
    for row in calls:
        first = cut.copy()
        first[1:] |= row[1:] != row[:-1]
        start = np.flatnonzero(first)
        end = np.r_[start[1:] - 1, L_u - 1]
        anc = row[start].astype(np.int64)
        ln = pos[end] - pos[start]
        tracts.append(np.column_stack([start, end, anc]).astype(np.int64))
        lengths.append(ln)
        b = np.searchsorted(edges, ln, side='right') - 1
        ok = (b >= 0) & (b < edges.size - 1)
        np.add.at(counts, (anc[ok], b[ok]), 1)
        np.add.at(sums, (anc[ok], b[ok]), ln[ok])
    return dict(tracts=tracts, lengths=lengths, hist=dict(edges=edges, counts=counts,
                                                          sum_len=sums))
