// The per-fit sums of m binomial GLMs with the logit link over one small design (the reference
// has no such analysis): what one Newton step of sim/glm.py needs that does not come from the
// genomes.  The dosages enter a logistic fit only through X^T D (gnx_assoc_cross); the score's
// other half, the information matrix and the log-likelihood's normaliser are functions of
// (X, beta_k) alone,
//
//   gnx_glm_sweep   sums fp64 [m][1 + p + p(p+1)/2] = [ s, A, I ] per fit (include/gnx_glm.h)
//
// k_glm_sweep<P> follows k_assoc_cross (gnx_assoc.hip) with the roles turned: lane = fit (its P
// coefficients and 1 + P + P(P+1)/2 accumulators stay in registers), block = 256 fits, and the
// design is what streams: tiles of GLM_TI rows of X are staged in LDS and every lane reads the
// same entries (broadcasts).  Each thread fetches its share of the next tile into registers
// before it works on the current one.  blockIdx.y = a stretch of individuals, whose partial sums
// go to Pt[stretch][fit][cols]; k_glm_sum adds the stretches in ascending order.  No atomics.
//
// The order of every sum is fixed by n alone (glm_stretch below), and nothing a lane computes
// depends on another lane, so a fit's sums depend neither on m, nor on its row in B, nor on the
// batch of fits it is worked off in.  P is a template parameter and every P in 1..8 is an
// instance of its own: none spills (DESIGN.md section 29 lists the registers), and padding to
// {2, 4, 8} would spend up to twice the fp64 FMAs (21 accumulators at p = 5 against 45).
#include <cmath>
#include "gnx_internal.h"
#include "../../include/gnx_glm.h"

#define GLM_TI 64                  // rows of X per LDS tile, and the unit of a stretch
#define GLM_FITS 256               // fits per block
#define GLM_PMAX 8
#define GLM_BUDGET (1ll << 30)     // bytes of partial sums per batch unless gnx_glm_budget says so

namespace {

// the stretches of individuals (documented in include/gnx_glm.h): at most 64, each a whole
// number of tiles
void glm_stretch(int64_t n, int64_t* per, int64_t* chunks) {
  const int64_t tiles = std::max<int64_t>(1, (n + GLM_TI - 1) / GLM_TI);
  const int64_t want = std::min<int64_t>(tiles, 64);
  const int64_t per_tiles = (tiles + want - 1) / want;
  *per = per_tiles * GLM_TI;
  *chunks = (n + *per - 1) / *per;
}

}  // namespace

template <int P>
__global__ void __launch_bounds__(GLM_FITS)
k_glm_sweep(int64_t n, int64_t per_chunk, int64_t m, const double* __restrict__ X,
            const double* __restrict__ B, double* __restrict__ Pt) {
  constexpr int NI = P * (P + 1) / 2, COLS = 1 + P + NI;
  constexpr int NF = (GLM_TI * P + GLM_FITS - 1) / GLM_FITS;    // entries of a tile per thread
  __shared__ double Xs[GLM_TI][P];
  const int tid = threadIdx.x;
  const int64_t k = (int64_t)blockIdx.x * GLM_FITS + tid;
  const int64_t i_begin = (int64_t)blockIdx.y * per_chunk;
  const int64_t i_end = min(n, i_begin + per_chunk);
  double beta[P], A[P], Iu[NI], s = 0.0;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    beta[j] = k < m ? B[k * P + j] : 0.0;
    A[j] = 0.0;
  }
#pragma unroll
  for (int q = 0; q < NI; ++q) Iu[q] = 0.0;
  // this thread's share of a tile, fetched while the tile before it is worked on: the tile's
  // rows are consecutive in X, so entry q of the tile is X[t0 P + q]
  double gx[NF];
  auto fetch = [&](int64_t t0) {
    const int tn = (int)min((int64_t)GLM_TI, i_end - t0);
#pragma unroll
    for (int u = 0; u < NF; ++u) {
      const int q = tid + GLM_FITS * u;
      gx[u] = q < tn * P ? X[t0 * P + q] : 0.0;
    }
  };
  if (i_begin < i_end) fetch(i_begin);
  for (int64_t t0 = i_begin; t0 < i_end; t0 += GLM_TI) {
    const int tn = (int)min((int64_t)GLM_TI, i_end - t0);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NF; ++u) {
      const int q = tid + GLM_FITS * u;
      if (q < GLM_TI * P) (&Xs[0][0])[q] = gx[u];
    }
    __syncthreads();
    if (t0 + GLM_TI < i_end) fetch(t0 + GLM_TI);
#pragma unroll 2
    for (int i = 0; i < tn; ++i) {
      double x[P];
#pragma unroll
      for (int j = 0; j < P; ++j) x[j] = Xs[i][j];
      double eta = 0.0;
#pragma unroll
      for (int j = 0; j < P; ++j) eta = fma(x[j], beta[j], eta);
      const double t = exp(-fabs(eta));
      const double r = 1.0 / (1.0 + t);
      const double tr = t * r;
      const double mu = eta >= 0.0 ? r : tr;
      const double w = tr * r;
      s += fmax(eta, 0.0) + log1p(t);
      int q = 0;
#pragma unroll
      for (int j = 0; j < P; ++j) {
        A[j] = fma(mu, x[j], A[j]);
        const double wx = w * x[j];
#pragma unroll
        for (int c = j; c < P; ++c) {
          Iu[q] = fma(wx, x[c], Iu[q]);
          ++q;
        }
      }
    }
  }
  if (k < m) {
    double* out = Pt + ((int64_t)blockIdx.y * m + k) * COLS;
    out[0] = s;
#pragma unroll
    for (int j = 0; j < P; ++j) out[1 + j] = A[j];
#pragma unroll
    for (int q = 0; q < NI; ++q) out[1 + P + q] = Iu[q];
  }
}

// the stretches added in ascending order: Z [M] from Pt [chunks][M], M = fits x cols
__global__ void k_glm_sum(int64_t M, int chunks, const double* __restrict__ Pt,
                          double* __restrict__ Z) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < M; t += stride) {
    double s = Pt[t];
    for (int q = 1; q < chunks; ++q) s += Pt[(int64_t)q * M + t];
    Z[t] = s;
  }
}

namespace {

void glm_launch(int p, dim3 grid, gnx_state* h, int64_t n, int64_t per, int64_t m,
                const double* d_X, const double* d_B, double* d_P) {
#define GLM_GO(P)                                                                              \
  case P:                                                                                      \
    hipLaunchKernelGGL((k_glm_sweep<P>), grid, dim3(GLM_FITS), 0, h->stream, n, per, m, d_X,   \
                       d_B, d_P);                                                              \
    break
  switch (p) {
    GLM_GO(1);
    GLM_GO(2);
    GLM_GO(3);
    GLM_GO(4);
    GLM_GO(5);
    GLM_GO(6);
    GLM_GO(7);
    GLM_GO(8);
  }
#undef GLM_GO
}

// the first entry of a [rows][p] that is not finite, or -1
int64_t glm_not_finite(const double* a, int64_t count) {
  for (int64_t t = 0; t < count; ++t)
    if (!std::isfinite(a[t])) return t;
  return -1;
}

}  // namespace

extern "C" int gnx_glm_budget(gnx_state* h, int64_t bytes) {
  if (bytes < 0) {
    gnx_set_error("gnx_glm_budget: bytes >= 0 (0: the default)");
    return 1;
  }
  h->glm_budget = bytes;
  return 0;
}

extern "C" int gnx_glm_sweep(gnx_state* h, int64_t n, int32_t p, const double* X, int64_t m,
                             const double* B, double* sums, int64_t* stretch,
                             int64_t* stretches, double* kernel_ms) {
  const char* who = "gnx_glm_sweep";
  if (stretch) *stretch = 0;
  if (stretches) *stretches = 0;
  if (kernel_ms) *kernel_ms = 0.0;
  if (p < 1 || p > GLM_PMAX) {
    gnx_set_error("%s: 1 <= p <= %d columns (got %d)", who, GLM_PMAX, p);
    return 1;
  }
  if (n < 1 || n > (1ll << 30)) {
    gnx_set_error("%s: 1..2^30 individuals (n = %lld)", who, (long long)n);
    return 1;
  }
  if (m < 1 || m > (1ll << 24)) {
    gnx_set_error("%s: 1..2^24 fits (m = %lld)", who, (long long)m);
    return 1;
  }
  if (!X || !B || !sums) {
    gnx_set_error("%s: null X, B or sums", who);
    return 1;
  }
  int64_t bad = glm_not_finite(X, n * p);
  if (bad >= 0) {
    gnx_set_error("%s: X is not finite (row %lld, column %lld)", who, (long long)(bad / p),
                  (long long)(bad % p));
    return 1;
  }
  bad = glm_not_finite(B, m * p);
  if (bad >= 0) {
    gnx_set_error("%s: B is not finite (fit %lld, column %lld)", who, (long long)(bad / p),
                  (long long)(bad % p));
    return 1;
  }
  const int64_t cols = 1 + p + p * (p + 1) / 2;
  int64_t per = 0, chunks = 0;
  glm_stretch(n, &per, &chunks);
  // the fits of one batch: a multiple of GLM_FITS whose partial sums fit the budget
  const int64_t budget = h->glm_budget > 0 ? h->glm_budget : GLM_BUDGET;
  int64_t mb = budget / (8 * cols * chunks) / GLM_FITS * GLM_FITS;
  mb = std::min<int64_t>(std::max<int64_t>(mb, GLM_FITS), (m + GLM_FITS - 1) / GLM_FITS * GLM_FITS);

  GnxScratch s(who);
  double *d_X = nullptr, *d_B = nullptr, *d_P = nullptr, *d_Z = nullptr;
  GNXCHK(s.get(&d_X, (size_t)n * p));
  GNXCHK(s.get(&d_B, (size_t)m * p));
  GNXCHK(s.get(&d_P, (size_t)chunks * std::min(mb, m) * cols));
  GNXCHK(s.get(&d_Z, (size_t)std::min(mb, m) * cols));
  GNXCHK(gnx_h2d(h, d_X, X, (size_t)n * p * sizeof(double)));
  GNXCHK(gnx_h2d(h, d_B, B, (size_t)m * p * sizeof(double)));
  double ms = 0.0;
  int64_t n_launch = 0;
  GnxCallTimer tm(h, &ms, &n_launch);
  for (int64_t k0 = 0; k0 < m; k0 += mb) {
    const int64_t mk = std::min(mb, m - k0);
    tm.start();
    glm_launch(p, dim3((unsigned)((mk + GLM_FITS - 1) / GLM_FITS), (unsigned)chunks), h, n, per,
               mk, d_X, d_B + k0 * p, d_P);
    hipLaunchKernelGGL(k_glm_sum, dim3(gnx_grid(mk * cols, 256, 256 * 64)), dim3(256), 0,
                       h->stream, mk * cols, (int)chunks, d_P, d_Z);
    HIPCHK(hipGetLastError());
    GNXCHK(tm.stop(2));
    GNXCHK(gnx_d2h(h, sums + k0 * cols, d_Z, (size_t)mk * cols * sizeof(double)));
  }
  if (stretch) *stretch = per;
  if (stretches) *stretches = chunks;
  if (kernel_ms) *kernel_ms = ms;
  return 0;
}
