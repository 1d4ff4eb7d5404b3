"""The cases the logistic-fit tests share (tests/test_glm_host.py on the CPU, tests/test_gpu_glm.py
on the device): designs and coefficients of the sweep cases, their reference in extended
precision with the weights of the a priori bound, the ordered restatement of the fits whose
every |eta| is beyond the underflow of exp, and dosages drawn from known clines.  Everything is
generated from seeds; results are cached and must not be changed."""
import functools

import numpy as np

from geonomics_amd.sim import glm as G

U53 = 2.0 ** -53

# (n, m, p) of the sweep cases.  With 64 rows of X per tile and at most 64 stretches
# (include/gnx_glm.h): n = 1 is one ragged tile; 63 and 129 end inside a tile; m = 65, 257 and
# 64 are a ragged block of fits, one lane into a second block, and a quarter block; (4161, 5, 4)
# is 66 tiles in 33 stretches of 128, the last one a tile and one individual.  Every p of 1..8
# is a compiled instance of its own, so every p appears
SWEEP_SHAPES = [(1, 1, 1), (63, 65, 2), (129, 257, 3), (300, 64, 8), (4161, 5, 4), (65, 3, 5),
                (130, 3, 6), (200, 4, 7)]
ETA_MAX = 40.0          # the regular fits' largest |eta| spans 0 .. ETA_MAX
ETA_HUGE = 1000.0       # every |eta| of the last fit (m >= 2) is at least this


def design(n, p, seed):
    """X [n][p]: mixed signs, the columns' scales spread over 10^-2 .. 10^2; |X[:, 0]| stays
    inside scale_0 x [0.5, 2], so that a fit on column 0 alone has no small |eta|"""
    rng = np.random.RandomState(seed)
    scale = 10.0 ** (np.linspace(-2.0, 2.0, p) if p > 1 else np.zeros(1))
    scale = scale[rng.permutation(p)]
    X = rng.standard_normal((n, p)) * scale
    X[:, 0] = rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 2.0, n) * scale[0]
    return X, scale


def huge_fit(X, scale, sign=1.0):
    """the coefficients of a fit whose every |eta| is at least ETA_HUGE, of both signs over the
    rows: column 0 alone, so that eta = fma(x_0, b_0, +0) is the rounded product and the other
    columns add zeros"""
    b = np.zeros(X.shape[1])
    b[0] = sign * 2.0 * ETA_HUGE / scale[0]
    return b


@functools.lru_cache(maxsize=None)
def sweep_case(n, m, p):
    """(X [n][p], B [m][p]) of one shape: the largest |eta| of fit k is ETA_MAX k / (m' - 1)
    over the m' regular fits (fit 0 is beta = 0; a single fit: ETA_MAX / 8), and with m >= 2 the last fit is huge_fit"""
    X, scale = design(n, p, 3000 + n + p)
    rng = np.random.RandomState(4000 + n + m)
    reg = m - 1 if m >= 2 else m
    B = rng.standard_normal((m, p)) / scale
    top = np.abs(X @ B[:reg].T).max(axis=0)
    want = np.array([ETA_MAX / 8.0])
    if reg > 1:
        want = ETA_MAX * np.arange(reg) / (reg - 1)
    B[:reg] *= (want / top)[:, None]
    if m >= 2:
        B[m - 1] = huge_fit(X, scale)
    X.setflags(write=False)
    B.setflags(write=False)
    return X, B


@functools.lru_cache(maxsize=None)
def sweep_reference(n, m, p):
    """the sums of sweep_case in np.longdouble, and per output the weights of the bound
    |o - o_ref| <= 2^-53 sum_i (stretch + stretches + c + (p + 1) H_i) |term_i|,
    H_i = sum_j |X_ij B_kj|: T0 = sum_i |term_i| and T1 = sum_i H_i |term_i|
    -> (ref, T0, T1), longdouble [m][n_cols(p)]"""
    X, B = sweep_case(n, m, p)
    ld = np.longdouble
    Xl, Bl = X.astype(ld), B.astype(ld)
    eta = Bl @ Xl.T
    H = np.abs(Bl) @ np.abs(Xl).T
    t = np.exp(-np.abs(eta))
    r = 1 / (1 + t)
    mu = np.where(eta >= 0, r, t * r)
    w = t * r * r
    terms = [np.maximum(eta, ld(0)) + np.log1p(t)]
    terms += [mu * Xl[None, :, j] for j in range(p)]
    terms += [w * Xl[None, :, j] * Xl[None, :, c] for j in range(p) for c in range(j, p)]
    ref = np.stack([a.sum(axis=1) for a in terms], axis=1)
    T0 = np.stack([np.abs(a).sum(axis=1) for a in terms], axis=1)
    T1 = np.stack([(H * np.abs(a)).sum(axis=1) for a in terms], axis=1)
    for a in (ref, T0, T1):
        a.setflags(write=False)
    return ref, T0, T1


def needed_c(sums, n, m, p):
    """the smallest c >= 0 with which `sums` of sweep_case(n, m, p) meets the bound of
    sweep_reference (0 where the summation allowance alone covers the difference)"""
    ref, T0, T1 = sweep_reference(n, m, p)
    stretch, stretches = G.stretch_rule(n)
    ok = _representable(sums, T0)
    err = np.abs(np.asarray(sums).astype(np.longdouble) - ref) / np.longdouble(U53)
    need = err - (stretch + stretches) * T0 - (p + 1) * T1
    return float(max(0.0, (need[ok] / T0[ok]).max())) if ok.any() else 0.0


def _representable(sums, T0):
    """the outputs the bound speaks of: those whose sum of |term| is a normal fp64 number.  The
    others (zeros; w x x at |eta| >= ETA_HUGE, where extended precision still holds e^-1000)
    must be exactly zero"""
    ok = T0 >= np.finfo(np.float64).tiny
    assert (np.asarray(sums)[~ok] == 0).all()
    return ok


def within_bound(sums, n, m, p, c):
    """the worst |o - o_ref| / bound over the outputs the bound speaks of"""
    ref, T0, T1 = sweep_reference(n, m, p)
    stretch, stretches = G.stretch_rule(n)
    ok = _representable(sums, T0)
    err = np.abs(np.asarray(sums).astype(np.longdouble) - ref)
    bound = np.longdouble(U53) * ((stretch + stretches + c) * T0 + (p + 1) * T1)
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


def ordered_sum(v, n):
    """sum of v [n] in the order of gnx_glm_sweep: within a stretch over ascending
    individuals from +0 (np.add.accumulate adds one after the other), then the stretches left
    to right"""
    stretch, stretches = G.stretch_rule(n)
    tot = None
    for q in range(stretches):
        part = np.add.accumulate(np.r_[0.0, v[q * stretch:(q + 1) * stretch]])[-1]
        tot = part if tot is None else tot + part
    return tot


def huge_expected(X, b):
    """the bytes gnx_glm_sweep owes a fit of huge_fit: eta = the rounded x_0 b_0, mu = 1 where
    eta > 0 and 0 elsewhere, w = 0, so s = sum max(eta, 0), A_j = sum mu x_j (both in the call's
    order; mu x_j is exact) and I = 0"""
    n, p = X.shape
    eta = X[:, 0] * b[0]
    assert (np.abs(eta) > 800.0).all()
    assert n == 1 or ((eta > 0).any() and (eta < 0).any())
    out = np.zeros(G.n_cols(p))
    out[0] = ordered_sum(np.maximum(eta, 0.0), n)
    for j in range(p):
        out[1 + j] = ordered_sum(np.where(eta > 0, X[:, j], 0.0), n)
    return out


# ---- clines -------------------------------------------------------------------------------
CLINE_SEED = 11


@functools.lru_cache(maxsize=None)
def clines(seed=CLINE_SEED, n=2000, L=40):
    """dosages drawn from known sigmoid clines along x in [0, 10]: centres in 3..7, widths in
    1..6, rising or falling -> dict(D [n][L], x [n], centre, width, sign [L])"""
    rng = np.random.RandomState(seed)
    x = rng.uniform(0.0, 10.0, n)
    centre = rng.uniform(3.0, 7.0, L)
    width = rng.uniform(1.0, 6.0, L)
    sign = rng.choice([-1.0, 1.0], L)
    P = 1.0 / (1.0 + np.exp(-4.0 * sign[None, :] * (x[:, None] - centre[None, :])
                            / width[None, :]))
    D = ((rng.uniform(size=(n, L)) < P).astype(np.int64)
         + (rng.uniform(size=(n, L)) < P).astype(np.int64))
    for a in (D, x, centre, width, sign):
        a.setflags(write=False)
    return dict(D=D, x=x, centre=centre, width=width, sign=sign)
