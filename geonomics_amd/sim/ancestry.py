"""Model-based ancestry: the admixture model of STRUCTURE (Pritchard et al. 2000) fitted by the
EM of FRAPPE (Tang et al. 2005) / ADMIXTURE (Alexander et al. 2009), accelerated by SQUAREM
(Varadhan & Roland 2008).  Individual i draws each of its two alleles at locus l from ancestral
population k with probability q_ik; that allele is 1 with probability f_kl.  With dosages
d in {0, 1, 2}, p = sum_k q_k f_k and r = sum_k q_k (1 - f_k) the log-likelihood is
sum_il d ln p + (2 - d) ln r.

One EM sweep needs, per genotype, u = d / p and v = (2 - d) / r and their sums along both axes
(include/gnx_hip.h, gnx_admix_sweep): A[i][k] = sum_l (u f_kl + v (1 - f_kl)),
B1[k][l] = sum_i u q_ik, B0[k][l] = sum_i v q_ik.  The device takes them from the bit-packed
genomes (csrc/gnx_admix.hip); brute_sweep restates them in numpy.  The update (em_update) and the
driver (fit) are written once and run on torch device tensors and on numpy arrays alike: the sweep
is passed in as a callable, as sim/pca.py takes its products.
"""
import math

import numpy as np

EPS = 1e-6          # F lives in [EPS, 1 - EPS], Q at or above EPS
MAX_K = 16          # gnx_admix_sweep's template instances


# ---------------------------------------------------------------- the sweep, restated
def _fsum_last(a):
    """the correctly rounded sums (math.fsum) over the last axis"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    flat = a.reshape(-1, a.shape[-1])
    if flat.shape[1] <= 32:                    # many short rows: tuples from the columns' lists
        rows = zip(*[flat[:, k].tolist() for k in range(flat.shape[1])])
    else:
        rows = flat.tolist()
    return np.fromiter(map(math.fsum, rows), dtype=np.float64,
                       count=flat.shape[0]).reshape(a.shape[:-1])


def used_loci(used, L):
    """ascending locus numbers of `used`: None (all L), a bool mask [L] or a list of loci"""
    if used is None:
        return np.arange(L, dtype=np.int64)
    u = np.asarray(used)
    if u.dtype == bool:
        if u.size != L:
            raise ValueError('used: a mask of %d entries, not L = %d' % (u.size, L))
        return np.flatnonzero(u).astype(np.int64)
    u = np.unique(u.astype(np.int64).ravel())
    if u.size and (u[0] < 0 or u[-1] >= L):
        raise ValueError('used: loci in 0..%d' % (L - 1))
    return u


def brute_sweep(D, Q, F, used=None, exact=True):
    """gnx_admix_sweep restated (include/gnx_hip.h): D [n][L] dosages in {0, 1, 2}, Q [n][K],
    F [K][L] indexed by genome locus, used: the loci that count (None: all; a bool mask or a
    list).  Per genotype p = sum_k q f, r = sum_k q g with g = 1 - f rounded to fp64, u = d / p,
    v = (2 - d) / r: each product and each quotient is one IEEE operation and, with exact=True,
    every sum - p and r over k, A over the 2 L_u terms u f and v g, B over the n terms u q (v q),
    the log-likelihood over its 2 n L_u terms - is the correctly rounded sum of its terms
    (math.fsum).  exact=False takes the same sums by matrix products in numpy's order (fast:
    for long fits).
    -> dict(A [n][K], B1 [K][L], B0 [K][L] (0 at unused loci), loglik, loglik_abs (the sum of
    the |terms| of loglik, for error bounds))"""
    D = np.asarray(D)
    Q = np.asarray(Q, dtype=np.float64)
    F = np.asarray(F, dtype=np.float64)
    n, L = D.shape
    K = Q.shape[1]
    if Q.shape != (n, K) or F.shape != (K, L):
        raise ValueError('Q %s and F %s do not fit D %s' % (Q.shape, F.shape, D.shape))
    loci = used_loci(used, L)
    Du = D[:, loci].astype(np.float64)
    Fu = F[:, loci]
    Gu = 1.0 - Fu
    if exact:
        p = _fsum_last(Q[:, None, :] * Fu.T[None, :, :])
        r = _fsum_last(Q[:, None, :] * Gu.T[None, :, :])
    else:
        p, r = Q @ Fu, Q @ Gu
    u = Du / p
    v = (2.0 - Du) / r
    with np.errstate(divide='ignore', invalid='ignore'):
        lt = np.concatenate([(Du * np.log(p)).ravel(), ((2.0 - Du) * np.log(r)).ravel()])
    B1 = np.zeros((K, L))
    B0 = np.zeros((K, L))
    if exact:
        A = _fsum_last(np.concatenate([u[:, None, :] * Fu[None, :, :],
                                       v[:, None, :] * Gu[None, :, :]], axis=2))
        B1[:, loci] = _fsum_last(Q.T[:, None, :] * u.T[None, :, :])
        B0[:, loci] = _fsum_last(Q.T[:, None, :] * v.T[None, :, :])
        ll = math.fsum(lt.tolist())
        ll_abs = math.fsum(np.abs(lt).tolist())
    else:
        A = u @ Fu.T + v @ Gu.T
        B1[:, loci] = Q.T @ u
        B0[:, loci] = Q.T @ v
        ll = float(lt.sum())
        ll_abs = float(np.abs(lt).sum())
    return dict(A=A, B1=B1, B0=B0, loglik=ll, loglik_abs=ll_abs)


def host_sweep(D, exact=False):
    """the sweep fit() takes, over the dosages D [n][L_u] on the host (every locus used)"""
    D = np.asarray(D)

    def sweep(Q, F, want_B=True, want_loglik=True):
        got = brute_sweep(D, Q, F, None, exact)
        return got['A'], got['B1'], got['B0'], got['loglik']

    return sweep


def device_sweep(dev, slots=None, loci=None, locus_mask=None, budget=None):
    """the sweep fit() takes, on a Device: Q [n][K] and F [K][L_u] torch fp64 tensors on its
    device; loci (ascending, with their mask) restricts the columns, F and B being scattered to
    and gathered from genome loci around the call"""
    import torch
    tdev = torch.device('cuda', int(dev.cfg.device))
    loci_t = None if loci is None else torch.as_tensor(np.asarray(loci, np.int64), device=tdev)

    def sweep(Q, F, want_B=True, want_loglik=True):
        if loci_t is not None:
            full = torch.full((F.shape[0], int(dev.L)), 0.5, dtype=torch.float64, device=tdev)
            full[:, loci_t] = F
            F = full
        got = dev.admix_sweep(Q, F, slots, locus_mask, want_loglik, budget, want_B)
        B1, B0 = got['B1'], got['B0']
        if want_B and loci_t is not None:
            B1, B0 = B1[:, loci_t], B0[:, loci_t]
        return got['A'], B1, B0, got['loglik']

    return sweep


# ---------------------------------------------------------------- the update
def _xp(a):
    if hasattr(a, 'detach'):
        import torch
        return torch
    return np


def _to_numpy(a):
    if hasattr(a, 'detach'):
        return a.detach().cpu().numpy()
    return np.asarray(a)


def project(Q, F, eps=EPS):
    """the nearest feasible state as the update clamps it: F into [eps, 1 - eps]; Q at or above
    eps, its rows renormalised"""
    xp = _xp(Q)
    Q = xp.clip(Q, eps, None)
    return Q / Q.sum(axis=1, keepdims=True), xp.clip(F, eps, 1.0 - eps)


def em_update(Q, F, A, B1, B0, L_u, eps=EPS, update_F=True):
    """one EM step from a sweep's numerators (FRAPPE / ADMIXTURE's EM):
        q' = q A / (2 L_u),    f' = f B1 / (f B1 + (1 - f) B0),
    f' clamped to [eps, 1 - eps], q' clamped below at eps and its rows renormalised.  F, B1 and
    B0 hold the L_u used loci only.  update_F=False holds F (projection; B1 and B0 may be None).
    numpy arrays or torch tensors -> (Q', F') of the same kind"""
    xp = _xp(Q)
    Qn = xp.clip(Q * A / (2.0 * L_u), eps, None)
    Qn = Qn / Qn.sum(axis=1, keepdims=True)
    if not update_F:
        return Qn, F
    num = F * B1
    return Qn, xp.clip(num / (num + (1.0 - F) * B0), eps, 1.0 - eps)


# ---------------------------------------------------------------- the driver
def check_K(K):
    if isinstance(K, bool) or int(K) != K or not 1 <= K <= MAX_K:
        raise ValueError('K: a number of ancestral populations in 1..%d (got %r)' % (MAX_K, K))
    return int(K)


def init_random(n, L_u, K, seed=None):
    """Dirichlet(1) rows for Q, F uniform in [0.1, 0.9]"""
    rng = np.random.RandomState(seed)
    return rng.dirichlet(np.ones(K), size=n), rng.uniform(0.1, 0.9, (K, L_u))


def init_pca_Q(pcs, K, floor=0.05):
    """Q from the first K - 1 genetic PCs (no clustering): column k is PC k min-max scaled to
    [0, 1], the last column one minus their mean; every entry is raised to `floor` and the rows
    are normalised"""
    pcs = np.asarray(pcs, dtype=np.float64)
    n = pcs.shape[0]
    if K == 1:
        return np.ones((n, 1))
    if pcs.ndim != 2 or pcs.shape[1] < K - 1:
        raise ValueError("init='pca': %d PCs are needed for K = %d (got %s)"
                         % (K - 1, K, pcs.shape))
    s = pcs[:, :K - 1]
    span = s.max(axis=0) - s.min(axis=0)
    s = (s - s.min(axis=0)) / np.where(span > 0, span, 1.0)
    Q = np.maximum(np.column_stack([s, 1.0 - s.mean(axis=1)]), floor)
    return Q / Q.sum(axis=1, keepdims=True)


def _check_init(Q0, F0, n, L_u, K, need_F=True):
    Q0 = np.array(Q0, dtype=np.float64)
    if Q0.shape != (n, K):
        raise ValueError('init: Q of shape %s, not (n, K) = (%d, %d)' % (Q0.shape, n, K))
    if not (np.isfinite(Q0).all() and (Q0 > 0).all() and (Q0 < 1).all()) and K > 1:
        raise ValueError('init: the entries of Q lie strictly inside (0, 1)')
    if K == 1 and not (Q0 > 0).all():
        raise ValueError('init: the entries of Q are positive')
    if not need_F:
        return Q0, None
    F0 = np.array(F0, dtype=np.float64)
    if F0.shape != (K, L_u):
        raise ValueError('init: F of shape %s, not (K, L_u) = (%d, %d)' % (F0.shape, K, L_u))
    if not (np.isfinite(F0).all() and (F0 > 0).all() and (F0 < 1).all()):
        raise ValueError('init: the entries of F lie strictly inside (0, 1)')
    return Q0, F0


def fit(sweep, n, L_u, K, init='random', seed=None, accelerate=True, tol=1e-4, max_sweeps=2000,
        fixed_F=None, pcs=None, put=None, loci=None, individs=None):
    """fit the admixture model by EM.  sweep(Q, F, want_B, want_loglik) -> (A, B1, B0, loglik)
    over n individuals and L_u loci (host_sweep, device_sweep); put(array) moves a numpy array
    to where the sweep wants it (None: numpy).

    init: 'random' (init_random from `seed`); 'pca' (Q from `pcs`, the first K - 1 genetic PCs
    [n][K - 1], by init_pca_Q, and F by one em_update from F = 0.5 with that Q held); or a pair
    of arrays (Q [n][K], F [K][L_u]) strictly inside (0, 1).
    fixed_F [K][L_u]: projection - F is held, only Q is fitted, the sweep's B is not asked for
    and the components keep the order of fixed_F.
    accelerate: SQUAREM, scheme S3, over the concatenated (Q, F): from theta0 two EM steps give
    theta1, theta2; with r = theta1 - theta0, v = (theta2 - theta1) - r and
    alpha = min(-1, -|r| / |v|) the point theta0 - 2 alpha r + alpha^2 v is projected into the
    feasible set (project) and followed by one stabilising EM step.  The result is accepted only
    if its log-likelihood is not below that of theta2; otherwise theta2 is kept.  So the trace
    of accepted log-likelihoods does not decrease (up to rounding).  A cycle is four sweeps (two
    of them without the log-likelihood, one without B), five when theta2 is kept; n_sweeps
    counts them all, and the last sweeps before max_sweeps are plain steps.
    The fit stops when an accepted step gains less than tol, or when max_sweeps are used up.
    -> dict(Q [n][K], F [K][L_u] (numpy), loci, individs, loglik (the trace), n_sweeps,
    converged, n_params = n (K - 1) + K L_u (n (K - 1) under fixed_F), aic = 2 n_params - 2 ll,
    bic = n_params ln(n L_u) - 2 ll).  Components are ordered by decreasing mean ancestry."""
    K = check_K(K)
    n, L_u = int(n), int(L_u)
    if n < 1 or L_u < 1:
        raise ValueError('fit: at least one individual and one locus (n = %d, L_u = %d)'
                         % (n, L_u))
    if isinstance(max_sweeps, bool) or int(max_sweeps) != max_sweeps or max_sweeps < 1:
        raise ValueError('max_sweeps: a positive number of sweeps (got %r)' % (max_sweeps,))
    if not float(tol) >= 0.0:
        raise ValueError('tol: a gain in log-likelihood >= 0 (got %r)' % (tol,))
    put = put or (lambda a: np.asarray(a, dtype=np.float64))
    hold = fixed_F is not None
    if hold:
        F0 = np.array(fixed_F, dtype=np.float64)
        if F0.shape != (K, L_u) or not (np.isfinite(F0).all() and (F0 > 0).all()
                                         and (F0 < 1).all()):
            raise ValueError('fixed_F: an array (K, L_u) = (%d, %d) strictly inside (0, 1)'
                             % (K, L_u))
    n_sweeps = 0

    def run(Q, F, want_B=True, want_ll=True):
        nonlocal n_sweeps
        n_sweeps += 1
        A, B1, B0, ll = sweep(Q, F, want_B and not hold, want_ll)
        return dict(Q=Q, F=F, A=A, B1=B1, B0=B0, ll=float(ll) if want_ll else None)

    def step(S):
        return em_update(S['Q'], S['F'], S['A'], S['B1'], S['B0'], L_u, update_F=not hold)

    if isinstance(init, str):
        if init == 'random':
            Q0, Fr = init_random(n, L_u, K, seed)
            F0 = F0 if hold else Fr
        elif init == 'pca':
            if pcs is None and K > 1:
                raise ValueError("init='pca' needs pcs, the first K - 1 genetic PCs")
            Q0 = init_pca_Q(np.zeros((n, 0)) if K == 1 else pcs, K)
            if not hold:
                S = run(put(Q0), put(np.full((K, L_u), 0.5)))
                F0 = _to_numpy(em_update(S['Q'], S['F'], S['A'], S['B1'], S['B0'], L_u)[1])
        else:
            raise ValueError("init: 'random', 'pca' or a pair of arrays (Q, F), not %r" % (init,))
    else:
        try:
            Qi, Fi = init
        except (TypeError, ValueError):
            raise ValueError("init: 'random', 'pca' or a pair of arrays (Q, F)") from None
        Q0, Fi = _check_init(Qi, Fi, n, L_u, K, need_F=not hold)
        F0 = F0 if hold else Fi
    Q0, F0 = project(np.asarray(Q0, np.float64), np.asarray(F0, np.float64))

    S0 = run(put(Q0), put(F0))
    trace = [S0['ll']]
    converged = False
    while n_sweeps < max_sweeps:
        cycle = accelerate and n_sweeps + 5 <= max_sweeps   # (else plain steps to the end)
        S1 = run(*step(S0), want_ll=not cycle)
        if not cycle:
            new = S1
        else:
            Q2, F2 = step(S1)
            rq, rf = S1['Q'] - S0['Q'], S1['F'] - S0['F']
            vq, vf = (Q2 - S1['Q']) - rq, (F2 - S1['F']) - rf
            rr = float((rq * rq).sum()) + float((rf * rf).sum())
            vv = float((vq * vq).sum()) + float((vf * vf).sum())
            alpha = -max(1.0, math.sqrt(rr / vv)) if vv > 0 else -1.0
            Qe, Fe = project(S0['Q'] - 2.0 * alpha * rq + alpha * alpha * vq,
                             S0['F'] - 2.0 * alpha * rf + alpha * alpha * vf)
            if hold:
                Fe = S0['F']
            # the stabilising step from the extrapolated point, evaluated; theta2's
            # log-likelihood costs a sweep without B, and a whole one only when theta2 is kept
            Ss = run(*step(run(Qe, Fe, want_ll=False)))
            ll2 = run(Q2, F2, want_B=False)['ll']
            new = Ss if Ss['ll'] >= ll2 else run(Q2, F2)
        gain = new['ll'] - S0['ll']
        S0 = new
        trace.append(S0['ll'])
        if gain < tol:
            converged = True
            break
    Q = _to_numpy(S0['Q']).astype(np.float64)
    F = _to_numpy(S0['F']).astype(np.float64)
    if not hold:
        order = np.argsort(-Q.mean(axis=0), kind='stable')
        Q, F = Q[:, order], F[order]
    n_params = n * (K - 1) + (0 if hold else K * L_u)
    ll = trace[-1]
    return dict(Q=Q, F=F, loci=loci, individs=individs, loglik=np.array(trace), n_sweeps=n_sweeps,
                converged=converged, n_params=n_params, aic=2.0 * n_params - 2.0 * ll,
                bic=n_params * math.log(n * L_u) - 2.0 * ll)


def match_components(Q, Q_true):
    """the mean correlation between the columns of Q and those of Q_true under the best
    matching of labels (all K! of them: K is small) -> (mean correlation, the matching)"""
    import itertools
    K = Q.shape[1]
    C = np.corrcoef(Q.T, Q_true.T)[:K, K:]
    best = max(itertools.permutations(range(K)),
               key=lambda pm: sum(C[pm[k], k] for k in range(K)))
    return float(np.mean([C[best[k], k] for k in range(K)])), list(best)


def planted_case(n, L, K, fst=0.2, seed=0):
    """a sample with a planted structure, for tests and benchmarks: ancestral frequencies are
    Balding-Nichols draws around p ~ U(0.1, 0.9) with the given Fst (f_kl ~ Beta(p (1 - Fst) /
    Fst, (1 - p) (1 - Fst) / Fst)); two thirds of the individuals are unadmixed (their
    populations in turn), one third have Dirichlet(1) ancestries; dosages are binomial(2, Q F)
    -> (D [n][L] int64, Q [n][K], F [K][L])"""
    rng = np.random.RandomState(seed)
    p = rng.uniform(0.1, 0.9, L)
    c = (1.0 - fst) / fst
    F = np.clip(rng.beta(p * c, (1.0 - p) * c, size=(K, L)), EPS, 1.0 - EPS)
    Q = np.zeros((n, K))
    pure = (2 * n) // 3
    Q[np.arange(pure), np.arange(pure) % K] = 1.0
    Q[pure:] = rng.dirichlet(np.ones(K), size=n - pure)
    D = rng.binomial(2, np.clip(Q @ F, 0.0, 1.0)).astype(np.int64)
    return D, Q, F
