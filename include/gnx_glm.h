/*
 * gnx_glm.h - C-ABI of libgnxhip.so, continued: the per-fit sums of a binomial GLM with the
 * logit link (csrc/gnx_glm.hip; the reference has no such analysis).  Conventions as
 * gnx_hip.h; geonomics_amd/_native.py reads the prototypes below as it reads that header's.
 */
#ifndef GNX_GLM_H
#define GNX_GLM_H

#include "gnx_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the sums of one Newton step of m logistic fits over one design (csrc/gnx_glm.hip) ----
 * X fp64 [n][p] (HOST) is the design, 1 <= p <= 8 columns, the same for every fit; B fp64
 * [m][p] (HOST) holds the coefficients of fit k in row k.  The call knows nothing of trials,
 * dosages, loci or genomes (the handle lends its stream; no precondition on its population).
 * For every fit k < m, with cols = 1 + p + p (p + 1) / 2, the HOST buffer sums fp64 [m][cols]
 * receives
 *   sums[k] = [ s, A_0 .. A_{p-1}, I_00, I_01, .., I_{p-1,p-1} ]   (I: the upper triangle,
 *   row-major), the sums over the individuals i < n of
 *     eta = sum_j X_ij B_kj, by fma in ascending j from +0,
 *     t = exp(-|eta|),  r = 1 / (1 + t),  mu = eta >= 0 ? r : t r,  w = t r r,
 *     s   += max(eta, 0) + log1p(t)                  (= log(1 + e^eta))
 *     A_j  = fma(mu, X_ij, A_j)
 *     I_jk = fma(w X_ij, X_ik, I_jk),  j <= k        (w X_ij rounded once).
 * All fp64; one exp and one log1p per element and neither overflows: |eta| may be anything
 * finite, and where exp(-|eta|) underflows to zero (|eta| > 745.2) t = 0, mu is exactly 0 or 1,
 * w = 0 and the element adds max(eta, 0) to s.
 * Order of the sums, fixed by n alone.  The individuals 0 .. n - 1 are cut into stretches of
 * `*stretch` consecutive ones, the last one ragged:
 *   tiles = ceil(n / 64),  per = ceil(tiles / min(tiles, 64)),
 *   *stretch = 64 per,  *stretches = ceil(n / *stretch).
 * Within a stretch every sum runs over ascending individuals from +0; the stretches' sums are
 * then added left to right from the first.  No atomics: a repeated call is byte-equal, and a
 * fit's sums depend neither on m nor on its row in B.  The partial sums take 8 cols m *stretches
 * bytes of device scratch; the fits are worked off in batches of a multiple of 256 whose partial
 * sums stay under gnx_glm_budget (at least 256 fits per batch), which changes no fit's sums.
 * *stretch, *stretches, *kernel_ms (each may be NULL): the rule's result and the HIP-event time
 * of the call's kernels.  Refused (return 1) before anything is launched: p outside 1..8, n
 * outside 1..2^30, m outside 1..2^24, a null X, B or sums, a NaN or infinity in X or B.       */
int gnx_glm_sweep(gnx_state* h, int64_t n, int32_t p, const double* X, int64_t m, const double* B,
                  double* sums, int64_t* stretch, int64_t* stretches, double* kernel_ms);
/* bytes of device scratch the partial sums of one batch of gnx_glm_sweep may take (0: the
 * default, 1 GiB); bytes < 0 is refused.  No output depends on it.                            */
int gnx_glm_budget(gnx_state* h, int64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GNX_GLM_H */
