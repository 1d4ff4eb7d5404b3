// Mantel tests and MMRR on the device (reference demos/_IBD_IBE.py:195-330: calc_dists, then
// data/IBD_IBE_demo/run_mantel.R, vegan's mantel.partial, and data/IBD_IBE_demo/MMRR.py:7-74,
// which refits an OLS on the n (n - 1) / 2 unfolded pairs once per permutation).  Permuting the
// rows and columns of the genetic distance matrix Y changes only the cross-sums
//
//   S_k(p) = sum over a > b of Y[a][b] * | f_k[perm[p][a]] - f_k[perm[p][b]] |
//
// (f_k: the per-individual columns of predictor k; perm[p][a]: whose columns individual a of
// the sample takes); every statistic follows from them and the fixed moments by fp64 algebra on
// the host (geonomics_amd/sim/mmrr.py).
//
//   gnx_dist_perm_sums       S [n_perm][n_pred] and the moments of the unpermuted sample, fp64
//   gnx_dist_perm_sums_mat   the same with n x n matrices as further predictors
//
// Both are mantel_sums, which takes column predictors (possibly none) and matrices (possibly
// none); the entries differ in whether they take matrices and in their name.
//
// Y[a][b] = 0.5 sqrt(G_aa + G_bb - 2 G_ab) of the exact Gram matrix (k_geno_gather, k_geno_gram
// into device scratch; G never leaves the device), the predictor distance = sqrt of the sum of
// the squared column differences, columns widened from fp32; products and sums in fp64, sqrt
// IEEE.  Nothing n x n is gathered per permutation: thread = permutation, and the permuted
// distance is recomputed from two short rows of the feature table F [n][D] (fp32, L2-resident).
//
// k_mantel_perm: block = MT_BLOCK permutations x one contiguous range of the 64 x 64 tiles of
// the lower triangle (t = ti (ti + 1) / 2 + tj, tj <= ti; the ranges of the MT_UNITS units
// differ by at most one tile, so the load is even without pairing strips).  A tile is worked
// off in stripes of JB columns: the stripe of Y (64 x JB, zero where a <= b or past n) is
// converted once into LDS and read by all lanes as a broadcast; every thread stages the columns
// of the stripe's JB individuals, taken through its own permutation, in its own LDS lane
// (Fb[j][c][thread]: consecutive lanes, consecutive banks), then walks the 64 rows, gathering
// each row's columns once.  The accumulators stay in registers over the whole range; one
// partial per (unit, permutation, predictor), added over the units in unit order by
// k_mantel_unit_sum: no atomics, so a call repeated is bit-equal.
//
// Matrix predictors (k_mantel_perm<MT_JB, true>): predictors n_pred .. n_pred + n_mat - 1 are
// n x n matrices on the device, x[a][b] = X[a][b], so the permuted distance is a gather
// X[perm a][perm b] and cannot be recomputed from two short rows.  The decomposition is the
// same; the pairs are walked with perm a fixed over the inner loop, so a thread gathers within
// one row of X, which L2 holds, at the stripe's permuted columns (Qb, staged once per stripe in
// LDS next to Fb).  With a matrix present a stripe is always MT_JB = 8 wide, without one it is
// 16 wide where the staged columns fit MT_FB and 8 otherwise.  A column predictor's terms are
// the same either way, added stripe by stripe: its sums in front of a matrix are the bits of
// the column-only call when that call's stripes are 8 wide too (more than 4 columns), and
// within the summation bound of them otherwise.  With no matrix gnx_dist_perm_sums_mat is
// gnx_dist_perm_sums.
#include "gnx_geno.h"

#define MT_BLOCK 128         // permutations (threads) per block
#define MT_UNITS 512         // tile ranges: the partial buffer is MT_UNITS x n_perm x n_pred
#define MT_PMAX 4            // predictors
#define MT_DMAX 8            // columns of all predictors together
#define MT_FB 8192           // floats of the staged stripe per block: JB x D x MT_BLOCK
#define MT_JB 8              // the stripe that fits MT_FB whatever D is: the matrix path's
#define MT_NMOM (2 + 2 * MT_PMAX + MT_PMAX * (MT_PMAX + 1) / 2)
#define MT_MBLOCK 128        // threads of the moments kernel

// what the kernels need to know about the predictors: predictor k owns columns
// off[k] .. off[k + 1] - 1 of F
struct MtPred {
  int n_pred;
  int D;
  int off[MT_PMAX + 1];
};

// the device column behind a (field, index) code
struct MtCols {
  const float* col[MT_DMAX];
};

// the matrix predictors, behind the column predictors
struct MtMat {
  int n_mat;
  const double* X[MT_PMAX];
};

// F[i][c] = column c of the individual in slot slots[i]
__global__ void k_mantel_features(int64_t n, int D, const int64_t* __restrict__ slots, MtCols C,
                                  float* __restrict__ F) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * D) return;
  const int64_t i = t / D;
  const int c = (int)(t - i * D);
  const float* src = C.col[0];
#pragma unroll
  for (int q = 1; q < MT_DMAX; ++q)
    if (c == q) src = C.col[q];
  F[t] = src[slots ? slots[i] : i];
}

// Y[a][b] of the sample, or 0 where the pair does not count (a <= b, or past n)
__device__ __forceinline__ double mt_y(const int64_t* __restrict__ G, int64_t n, int64_t a,
                                       int64_t b) {
  if (a >= n || b >= a) return 0.0;
  const int64_t d2 = G[a * n + a] + G[b * n + b] - 2 * G[a * n + b];
  return 0.5 * sqrt((double)d2);
}

__device__ __forceinline__ void mt_tile_of(int64_t t, int& ti, int& tj) {
  int r = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((int64_t)r * (r + 1) / 2 > t) --r;
  while ((int64_t)(r + 1) * (r + 2) / 2 <= t) ++r;
  ti = r;
  tj = (int)(t - (int64_t)r * (r + 1) / 2);
}

// what a thread keeps in its LDS lane beside Fb: the column path the row's columns, the matrix
// path the stripe's permuted columns; neither instantiation carries the other's array
template <int JB, bool MAT>
struct MtLanes {
  float Fa[MT_DMAX][MT_BLOCK];
};
template <int JB>
struct MtLanes<JB, true> {
  int32_t Qb[JB][MT_BLOCK];
};

template <int JB, bool MAT>
__global__ void __launch_bounds__(MT_BLOCK)
k_mantel_perm(int64_t n, int n_perm, int64_t n_tiles, int units, MtPred P, MtMat M,
              const int64_t* __restrict__ G, const float* __restrict__ F,
              const int32_t* __restrict__ permT, double* __restrict__ part) {
  static_assert(JB * MT_DMAX * MT_BLOCK <= MT_FB || !MAT, "the matrix path takes any D");
  __shared__ double Ys[64][JB];
  __shared__ float Fb[MT_FB];
  __shared__ MtLanes<JB, MAT> S;
  const int tid = threadIdx.x;
  const int D = P.D;
  const int K = MAT ? P.n_pred + M.n_mat : P.n_pred;
  const int p_raw = blockIdx.y * MT_BLOCK + tid;
  const int p = min(p_raw, n_perm - 1);            // idle lanes repeat the last permutation
  const int64_t t_begin = n_tiles * blockIdx.x / units;
  const int64_t t_end = n_tiles * (blockIdx.x + 1) / units;
  double acc[MT_PMAX];
  [[maybe_unused]] double accm[MAT ? MT_PMAX : 1];   // the matrices' sums
#pragma unroll
  for (int k = 0; k < MT_PMAX; ++k) {
    acc[k] = 0.0;
    if constexpr (MAT) accm[k] = 0.0;
  }
  int ti, tj;
  mt_tile_of(t_begin, ti, tj);
  for (int64_t t = t_begin; t < t_end; ++t) {
    const int64_t i0 = (int64_t)ti * 64, j0 = (int64_t)tj * 64;
    const int rows = (int)min((int64_t)64, n - i0);
    for (int jb = 0; jb < 64 && j0 + jb < n; jb += JB) {
      __syncthreads();                             // the last stripe's Ys has been read
      for (int q = tid; q < 64 * JB; q += MT_BLOCK) {
        const int a = q / JB, j = q - a * JB;
        Ys[a][j] = mt_y(G, n, i0 + a, j0 + jb + j);
      }
#pragma unroll
      for (int j = 0; j < JB; ++j) {
        const int64_t b = j0 + jb + j;
        const int32_t qb = b < n ? permT[b * n_perm + p] : -1;
        if constexpr (MAT) S.Qb[j][tid] = qb;
        for (int c = 0; c < D; ++c)
          Fb[(j * D + c) * MT_BLOCK + tid] = qb >= 0 ? F[(int64_t)qb * D + c] : 0.f;
      }
      __syncthreads();
      // on the diagonal tile rows at or before the stripe's first column hold no pair
      const int a_first = ti == tj ? jb + 1 : 0;
      for (int a = a_first; a < rows; ++a) {
        const int64_t qa = permT[(i0 + a) * n_perm + p];
        if constexpr (!MAT)
          for (int c = 0; c < D; ++c) S.Fa[c][tid] = F[qa * D + c];
#pragma unroll
        for (int k = 0; k < MT_PMAX; ++k) {
          if (k < P.n_pred) {
            double s[JB];
#pragma unroll
            for (int j = 0; j < JB; ++j) s[j] = 0.0;
            for (int c = P.off[k]; c < P.off[k + 1]; ++c) {
              double fa;
              if constexpr (MAT) fa = (double)F[qa * D + c];
              else fa = (double)S.Fa[c][tid];
#pragma unroll
              for (int j = 0; j < JB; ++j) {
                const double d = fa - (double)Fb[(j * D + c) * MT_BLOCK + tid];
                s[j] += d * d;
              }
            }
#pragma unroll
            for (int j = 0; j < JB; ++j) acc[k] += Ys[a][j] * sqrt(s[j]);
          }
        }
        if constexpr (MAT) {
#pragma unroll
          for (int k = 0; k < MT_PMAX; ++k) {
            if (k < M.n_mat) {
              const double* __restrict__ row = M.X[k] + qa * n;
#pragma unroll
              for (int j = 0; j < JB; ++j) {
                const int32_t qb = S.Qb[j][tid];
                accm[k] += Ys[a][j] * (qb >= 0 ? row[qb] : 0.0);
              }
            }
          }
        }
      }
    }
    if (++tj > ti) {
      ++ti;
      tj = 0;
    }
  }
  if (p_raw < n_perm) {
    double* o = part + ((int64_t)blockIdx.x * n_perm + p_raw) * K;
#pragma unroll
    for (int k = 0; k < MT_PMAX; ++k) {
      if (k < P.n_pred) o[k] = acc[k];
      if constexpr (MAT)
        if (k < M.n_mat) o[P.n_pred + k] = accm[k];
    }
  }
}

// out[q] = the units' partials of (permutation, predictor) q, added in unit order
__global__ void k_mantel_unit_sum(int64_t m, int units, const double* __restrict__ part,
                                  double* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= m) return;
  double s = 0.0;
  for (int u = 0; u < units; ++u) s += part[(int64_t)u * m + q];
  out[q] = s;
}

// The moments of the unpermuted sample over the pairs a > b: block = one range of tiles (as
// above), thread = the entries tid, tid + MT_MBLOCK, ... of each tile in that order, the block
// adds its threads by a fixed tree.  mom[unit][MT_NMOM] = sum y, sum y^2, sum x_k [MT_PMAX],
// sum y x_k [MT_PMAX], sum x_k x_l (k <= l, row-major); the host adds the units in order.
// Predictor k >= n_pred is matrix k - n_pred: x = X[a][b].
__global__ void __launch_bounds__(MT_MBLOCK)
k_mantel_moments(int64_t n, int64_t n_tiles, int units, MtPred P, MtMat M,
                 const int64_t* __restrict__ G, const float* __restrict__ F,
                 double* __restrict__ mom) {
  __shared__ double red[MT_MBLOCK][MT_NMOM];
  const int tid = threadIdx.x;
  const int D = P.D;
  const int64_t t_begin = n_tiles * blockIdx.x / units;
  const int64_t t_end = n_tiles * (blockIdx.x + 1) / units;
  double m[MT_NMOM];
#pragma unroll
  for (int c = 0; c < MT_NMOM; ++c) m[c] = 0.0;
  int ti, tj;
  mt_tile_of(t_begin, ti, tj);
  for (int64_t t = t_begin; t < t_end; ++t) {
    for (int q = tid; q < 64 * 64; q += MT_MBLOCK) {
      const int64_t a = (int64_t)ti * 64 + (q >> 6), b = (int64_t)tj * 64 + (q & 63);
      if (a >= n || b >= a) continue;
      const double y = mt_y(G, n, a, b);
      double x[MT_PMAX];
#pragma unroll
      for (int k = 0; k < MT_PMAX; ++k) {
        double v = 0.0;
        if (k < P.n_pred) {
          double s = 0.0;
          for (int c = P.off[k]; c < P.off[k + 1]; ++c) {
            const double d = (double)F[a * D + c] - (double)F[b * D + c];
            s += d * d;
          }
          v = sqrt(s);
        } else if (k - P.n_pred < M.n_mat) {
          const double* X = M.X[0];
#pragma unroll
          for (int q2 = 1; q2 < MT_PMAX; ++q2)
            if (k - P.n_pred == q2) X = M.X[q2];
          v = X[a * n + b];
        }
        x[k] = v;
      }
      m[0] += y;
      m[1] += y * y;
      int at = 2 + 2 * MT_PMAX;
#pragma unroll
      for (int k = 0; k < MT_PMAX; ++k) {
        m[2 + k] += x[k];
        m[2 + MT_PMAX + k] += y * x[k];
#pragma unroll
        for (int l = k; l < MT_PMAX; ++l) m[at++] += x[k] * x[l];
      }
    }
    if (++tj > ti) {
      ++ti;
      tj = 0;
    }
  }
#pragma unroll
  for (int c = 0; c < MT_NMOM; ++c) red[tid][c] = m[c];
  __syncthreads();
  for (int d = MT_MBLOCK / 2; d > 0; d >>= 1) {
    if (tid < d)
#pragma unroll
      for (int c = 0; c < MT_NMOM; ++c) red[tid][c] += red[tid + d][c];
    __syncthreads();
  }
  if (tid < MT_NMOM) mom[blockIdx.x * MT_NMOM + tid] = red[0][tid];
}

namespace {

// the call behind both entries: n_pred column predictors (possibly none), then n_mat matrices
// (possibly none); rule: how the entry words the count it accepts
int mantel_sums(gnx_state* h, const char* who, const char* rule, int64_t n, const int64_t* slots,
                const uint64_t* locus_mask, int32_t n_pred, const int32_t* pred_off,
                const int32_t* pred_cols, int32_t n_mat, const double* mats, int32_t n_perm,
                const int32_t* perm, double* sums, double* moments) {
  GNXCHK(geno_ready(h, who));
  if (n < 1 || n > 8192) {
    gnx_set_error("%s: 1..8192 individuals per call (the matrix is n x n)", who);
    return 1;
  }
  if (n_pred < 0 || n_mat < 0 || n_pred + n_mat < 1 || n_pred + n_mat > MT_PMAX ||
      (n_pred > 0 && (!pred_off || !pred_cols)) || (n_mat > 0 && !mats)) {
    gnx_set_error("%s: 1..%d predictors%s", who, MT_PMAX, rule);
    return 1;
  }
  if (n_perm < 1 || n_perm > (1 << 20) || !perm || !sums || !moments) {
    gnx_set_error("%s: 1..2^20 permutations, and non-null perm, sums and moments", who);
    return 1;
  }
  const int K = n_pred + n_mat;
  // the predictors' columns
  MtPred P = {};
  MtCols C = {};
  MtMat M = {};
  P.n_pred = n_pred;
  M.n_mat = n_mat;
  const GnxSoA a = h->soa[h->cur];
  const int64_t cap = h->cfg.cap_inds;
  if (n_pred > 0 && pred_off[0] != 0) {
    gnx_set_error("%s: pred_off starts at 0", who);
    return 1;
  }
  for (int k = 0; k < n_pred; ++k) {
    if (pred_off[k + 1] <= pred_off[k] || pred_off[k + 1] > MT_DMAX) {
      gnx_set_error("%s: every predictor has at least one column, all together at most %d", who,
                    MT_DMAX);
      return 1;
    }
    P.off[k + 1] = pred_off[k + 1];
  }
  P.D = n_pred > 0 ? pred_off[n_pred] : 0;
  for (int c = 0; c < P.D; ++c) {
    const int field = pred_cols[2 * c], idx = pred_cols[2 * c + 1];
    if (field == GNX_F_X && idx == 0) C.col[c] = a.x;
    else if (field == GNX_F_Y && idx == 0) C.col[c] = a.y;
    else if (field == GNX_F_E && idx >= 0 && idx < h->cfg.n_layers) C.col[c] = a.e + idx * cap;
    else if (field == GNX_F_Z && idx >= 0 && idx < h->cfg.n_traits) C.col[c] = a.z + idx * cap;
    else {
      gnx_set_error("%s: column %d: GNX_F_X, GNX_F_Y, a layer 0..%d of GNX_F_E or a trait 0..%d "
                    "of GNX_F_Z", who, c, h->cfg.n_layers - 1, h->cfg.n_traits - 1);
      return 1;
    }
  }
  for (int c = P.D; c < MT_DMAX; ++c) C.col[c] = P.D > 0 ? C.col[0] : a.x;
  // the matrices: finite, symmetric, zero on the diagonal (64 x 64 blocks, so that the transposed
  // reads stay in cache)
  for (int k = 0; k < n_mat; ++k) {
    const double* X = mats + (size_t)k * n * n;
    for (int64_t i = 0; i < n; ++i)
      if (X[i * n + i] != 0.0) {
        gnx_set_error("%s: matrix %d: the diagonal entry [%lld][%lld] = %g is not 0", who, k,
                      (long long)i, (long long)i, X[i * n + i]);
        return 1;
      }
    for (int64_t ib = 0; ib < n; ib += 64)
      for (int64_t jb = 0; jb <= ib; jb += 64)
        for (int64_t i = ib; i < std::min<int64_t>(ib + 64, n); ++i)
          for (int64_t j = jb; j < std::min<int64_t>(jb + 64, i); ++j) {
            const double u = X[i * n + j], v = X[j * n + i];
            if (!std::isfinite(u) || !std::isfinite(v)) {
              gnx_set_error("%s: matrix %d: a non-finite entry at [%lld][%lld]", who, k,
                            (long long)i, (long long)j);
              return 1;
            }
            if (u != v) {
              gnx_set_error("%s: matrix %d is not symmetric at [%lld][%lld]", who, k,
                            (long long)i, (long long)j);
              return 1;
            }
          }
  }
  // perm -> permT[a][p], checked for range before anything indexes with it
  std::vector<int32_t> permT((size_t)n * n_perm);
  for (int64_t p = 0; p < n_perm; ++p)
    for (int64_t i = 0; i < n; ++i) {
      const int32_t q = perm[p * n + i];
      if (q < 0 || q >= n) {
        gnx_set_error("%s: perm[%lld][%lld] = %d is not in 0..n-1", who, (long long)p,
                      (long long)i, q);
        return 1;
      }
      permT[(size_t)i * n_perm + p] = q;
    }
  GnxScratch s(who);
  int32_t* d_rows = nullptr;
  int64_t *d_slots = nullptr, *d_G = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows, &d_slots));
  GNXCHK(geno_gram_dev(h, s, d_rows, n, locus_mask, &d_G));
  const int T = (int)((n + 63) / 64);
  const int64_t n_tiles = (int64_t)T * (T + 1) / 2;
  const int units = (int)std::min<int64_t>(n_tiles, MT_UNITS);
  const int64_t m_out = (int64_t)n_perm * K;
  int32_t* d_permT = nullptr;
  float* d_F = nullptr;
  double *d_part = nullptr, *d_sums = nullptr, *d_mom = nullptr, *d_mats = nullptr;
  GNXCHK(s.get(&d_F, (size_t)n * P.D));
  GNXCHK(s.get(&d_permT, permT.size()));
  GNXCHK(s.get(&d_part, (size_t)units * m_out));
  GNXCHK(s.get(&d_sums, (size_t)m_out));
  GNXCHK(s.get(&d_mom, (size_t)units * MT_NMOM));
  GNXCHK(gnx_h2d(h, d_permT, permT.data(), permT.size() * sizeof(int32_t)));
  if (n_mat > 0) {
    GNXCHK(s.get(&d_mats, (size_t)n_mat * n * n));
    GNXCHK(gnx_h2d(h, d_mats, mats, (size_t)n_mat * n * n * sizeof(double)));
  }
  for (int k = 0; k < MT_PMAX; ++k)
    M.X[k] = d_mats + (size_t)(k < n_mat ? k : 0) * n * n;
  if (P.D > 0)
    hipLaunchKernelGGL(k_mantel_features, dim3(gnx_grid(n * P.D, 256)), dim3(256), 0, h->stream,
                       n, P.D, d_slots, C, d_F);
  hipLaunchKernelGGL(k_mantel_moments, dim3(units), dim3(MT_MBLOCK), 0, h->stream, n, n_tiles,
                     units, P, M, d_G, d_F, d_mom);
  // with a matrix MT_JB columns a stripe; without one the widest stripe whose staged columns fit
  // MT_FB floats (MT_JB x MT_DMAX x MT_BLOCK does)
  auto k_perm = k_mantel_perm<MT_JB, true>;
  if (n_mat == 0 && 16 * P.D * MT_BLOCK <= MT_FB) k_perm = k_mantel_perm<16, false>;
  else if (n_mat == 0) k_perm = k_mantel_perm<MT_JB, false>;
  hipLaunchKernelGGL(k_perm, dim3(units, (n_perm + MT_BLOCK - 1) / MT_BLOCK), dim3(MT_BLOCK), 0,
                     h->stream, n, n_perm, n_tiles, units, P, M, d_G, d_F, d_permT, d_part);
  hipLaunchKernelGGL(k_mantel_unit_sum, dim3(gnx_grid(m_out, 256)), dim3(256), 0, h->stream,
                     m_out, units, d_part, d_sums);
  HIPCHK(hipGetLastError());
  std::vector<double> mom((size_t)units * MT_NMOM);
  GNXCHK(gnx_d2h(h, mom.data(), d_mom, mom.size() * sizeof(double)));
  double tot[MT_NMOM] = {};
  for (int u = 0; u < units; ++u)
    for (int c = 0; c < MT_NMOM; ++c) tot[c] += mom[(size_t)u * MT_NMOM + c];
  // m, sum y, sum y^2, sum x_k, sum y x_k, sum x_k x_l (k <= l) of the K predictors
  double* o = moments;
  *o++ = (double)(n * (n - 1) / 2);
  *o++ = tot[0];
  *o++ = tot[1];
  for (int k = 0; k < K; ++k) *o++ = tot[2 + k];
  for (int k = 0; k < K; ++k) *o++ = tot[2 + MT_PMAX + k];
  int at = 2 + 2 * MT_PMAX;
  for (int k = 0; k < MT_PMAX; ++k)
    for (int l = k; l < MT_PMAX; ++l, ++at)
      if (k < K && l < K) *o++ = tot[at];
  return gnx_d2h(h, sums, d_sums, (size_t)m_out * sizeof(double));
}

}  // namespace

extern "C" int gnx_dist_perm_sums(gnx_state* h, int64_t n, const int64_t* slots,
                                  const uint64_t* locus_mask, int32_t n_pred,
                                  const int32_t* pred_off, const int32_t* pred_cols,
                                  int32_t n_perm, const int32_t* perm, double* sums,
                                  double* moments) {
  // (without matrices the count's rule is n_pred in 1..MT_PMAX with non-null tables)
  return mantel_sums(h, "gnx_dist_perm_sums", "", n, slots, locus_mask, n_pred, pred_off,
                     pred_cols, 0, nullptr, n_perm, perm, sums, moments);
}

extern "C" int gnx_dist_perm_sums_mat(gnx_state* h, int64_t n, const int64_t* slots,
                                      const uint64_t* locus_mask, int32_t n_pred,
                                      const int32_t* pred_off, const int32_t* pred_cols,
                                      int32_t n_mat, const double* mats, int32_t n_perm,
                                      const int32_t* perm, double* sums, double* moments) {
  return mantel_sums(h, "gnx_dist_perm_sums_mat", ", columns and matrices together", n, slots,
                     locus_mask, n_pred, pred_off, pred_cols, n_mat, mats, n_perm, perm, sums,
                     moments);
}
