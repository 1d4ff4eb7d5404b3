/*
 * gnx_ldwin.h - C-ABI of libgnxhip.so, continued: linkage disequilibrium of every locus with
 * the loci inside a window around it (csrc/gnx_ldwin.hip; the reference has no such analysis).
 * Conventions as gnx_hip.h; geonomics_amd/_native.py reads the prototypes below as it reads
 * that header's.
 */
#ifndef GNX_LDWIN_H
#define GNX_LDWIN_H

#include "gnx_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- windowed r^2 per locus and per pair (csrc/gnx_ldwin.hip) ----------------------------
 * The sample (n, slots), loci int32 [n_loci] distinct, pos fp64 [n_loci] finite and
 * non-decreasing along the request, min_minor, *work, max_work and c1 int64 [n_loci] are those
 * of gnx_ld_bins: the chromosomes are 2 i + hom over the sample in its order, c_j = the 1-alleles
 * of loci[j] among the N = 2 n chromosomes, locus j is KEPT iff min(c_j, N - c_j) >=
 * max(1, min_minor), and for two kept loci, with c_ij the chromosomes that carry both,
 *   Dn = N c_ij - c_i c_j (int64),  r2 = (Dn Dn) / ((c_i (N - c_i)) (c_j (N - c_j)))
 * in fp64: the two integers of the denominator converted exactly, then one rounding each for
 * Dn Dn, the denominator's product and the quotient, no contraction.  Request indices i < j,
 * both kept, are IN THE WINDOW iff pos[j] - pos[i] <= window (fp64, one rounding, inclusive;
 * window may be +inf).
 *   partners[j] (int64 [n_loci] or NULL) = the kept loci k != j in the window of j on either
 *     side; 0 for a locus that is not kept.  Exact.
 *   score[j] (fp64 [n_loci] or NULL) = the sum of r2_jk over those partners; 0 for a locus that
 *     is not kept.  Order of the sum, fixed by the request alone (not by gnx_ld_budget): the
 *     request is cut into tiles of 64 consecutive indices; the tile pairs (ti <= tj) that hold
 *     an in-window pair are taken in ascending (ti, tj); within a tile pair a locus of ti adds
 *     its 64 columns as sum_{x < 16} (((t[x] + t[x + 16]) + t[x + 32]) + t[x + 48]) joined by an
 *     xor butterfly over x (8, 4, 2, 1), a locus of tj its 64 rows as sum_{y < 16} ascending of
 *     (((t[y] + t[y + 16]) + t[y + 32]) + t[y + 48]) (pairs outside the window or not kept
 *     add +0); on the diagonal the row sum comes before the column sum.  The tile pairs' sums
 *     of a locus are added from +0 left to right.  No atomics: a repeated call is bit-equal.
 *   Edges, when max_edges > 0 (at most 2^26): every in-window pair with r2 >= r2_min as
 *     (ei[k], ej[k], er2[k]), ei < ej request indices, sorted by (ei, ej); *n_edges = their
 *     number.  More than max_edges: return 1 with *n_edges = the number found and the message
 *     "... exceed max_edges ..." (nothing else is written), as gnx_kin_pairs does with
 *     max_pairs.  max_edges == 0: no list; n_edges, ei, ej, er2 may be NULL.
 * *work = the listed tile pairs x ceil(N / 64) chromosome words; max_work <= 0: only *work is
 * computed and nothing is launched; *work > max_work is refused.  The bit rows of a stretch of
 * consecutive tiles together with the tiles their windows reach (one buffer) and the stretch's
 * per-tile-pair partial sums (1 KiB each) stay under gnx_ld_budget bytes; a request whose first
 * tile with its reach alone does not fit is refused with the bytes it needs.  No output depends
 * on the budget.  Refused (return 1) before anything is launched: what gnx_ld_bins refuses of
 * the sample, loci and pos; window negative or NaN; r2_min outside 0..1 or NaN; max_edges
 * outside 0..2^26; a null work, c1 or (max_edges > 0) edge output.  The call reads the genomes
 * and changes nothing in the handle but the figures of gnx_ld_window_info.                    */
int gnx_ld_window(gnx_state* h, int64_t n, const int64_t* slots, int32_t n_loci,
                  const int32_t* loci, const double* pos, double window, int32_t min_minor,
                  double r2_min, int64_t max_edges, int64_t max_work, int64_t* work, int64_t* c1,
                  int64_t* partners, double* score, int64_t* n_edges, int32_t* ei, int32_t* ej,
                  double* er2);
/* of the last gnx_ld_window: the HIP-event time of its kernels, their number, and the stretches
 * of tiles the loci were worked off in (each may be NULL)                                     */
int gnx_ld_window_info(gnx_state* h, double* kernel_ms, int64_t* launches, int64_t* locus_blocks);

#ifdef __cplusplus
}
#endif
#endif /* GNX_LDWIN_H */
