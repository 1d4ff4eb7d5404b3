// Per-locus association scans on the device (the reference has no such analysis): the
// cross-products of the dosage matrix D (d = a + b in {0, 1, 2}, a and b the bits of homologues 0
// and 1) with a host matrix Y in fp64, and the per-locus integer moments of d, in one pass over
// the bit-packed genomes.
//
//   gnx_assoc_cross   DtY = D_S^T Y fp64 [L][m], s1 = sum d, s2 = sum d^2 int64 [L], 1 <= m <= 32
//
// k_assoc_cross is k_geno_rmatmul (gnx_geno.hip) with fp64 accumulators: block = one 128-byte
// line of the genome (16 words, 1024 loci), wave v owns words 4v..4v+3, lane = locus within the
// word, so every (locus, column) of the block has one owner and no atomics are needed.  Tiles of
// AS_TI individuals are staged in LDS (their 16 words per homologue and their rows of Y); every
// lane of a half-wave reads the same entries (broadcasts): the word's 32-bit half that holds the
// lane's locus, then one v_bfe per homologue.  Each thread fetches its share of the next tile
// into registers before it works on the current one, so the dependent loads through the block
// table run beside the FMAs.  blockIdx.y = a stretch of individuals, whose partial sums go to
// P[stretch][L][m]; blockIdx.z = the chunk of MC columns.  k_assoc_sum adds the stretches in
// ascending order.
//
// The order of every sum is fixed by (n, L) alone (assoc_stretch below): within a stretch
// acc = fma(d, y, acc) over ascending individuals from +0, and d * y is exact, so the fma is the
// rounded sum acc + d y; then the stretches left to right.  A column's sums depend neither on the
// other columns nor on the column chunk, so m = 1 gives the bytes of the same vector sent as one
// of 32.  The integers are counted in the same loop by the blocks of column chunk 0 (the INTS
// instance, a launch of its own): s1 = sum d, s2 = s1 + 2 sum (d >> 1), d >> 1 being a & b.
#include "gnx_geno.h"

#define AS_TI 64       // individuals per LDS tile, and the unit of a stretch
#define AS_MMAX 32

namespace {

// The stretches of individuals (documented in include/gnx_hip.h): as many as fill the device
// (about 2048 blocks over the lines of 1024 loci), at most 32, each a whole number of tiles.
void assoc_stretch(int64_t n, int W64, int64_t* per, int* chunks) {
  const int lines = (W64 + 15) / 16;
  const int64_t tiles = std::max<int64_t>(1, (n + AS_TI - 1) / AS_TI);
  const int64_t want = std::min<int64_t>(std::min<int64_t>(tiles, 32), std::max(1, 2048 / lines));
  const int64_t per_tiles = (tiles + want - 1) / want;
  *per = per_tiles * AS_TI;
  *chunks = (int)((tiles + per_tiles - 1) / per_tiles);
}

}  // namespace

template <int MC, bool INTS>
__global__ void __launch_bounds__(256)
k_assoc_cross(int64_t n, int64_t per_chunk, int W64, int L, int m,
              const int32_t* __restrict__ rows, const u64* __restrict__ G, GnxHalves H,
              const double* __restrict__ Yin, double* __restrict__ P,
              uint32_t* __restrict__ PI) {
  __shared__ u64 Ws[AS_TI][2][16];
  __shared__ double Ys[AS_TI][MC];
  const int tid = threadIdx.x, lane = tid & 63, v = tid >> 6;
  const int wg = blockIdx.x * 16;                       // first word of the block's line
  const int c0 = (INTS ? 0 : 1 + blockIdx.z) * MC;      // INTS: the launch of column chunk 0
  const int64_t i_begin = (int64_t)blockIdx.y * per_chunk;
  const int64_t i_end = min(n, i_begin + per_chunk);
  // the 32-bit half of word 4v + u that holds this lane's locus, and the bit within it
  const uint32_t* W32 = (const uint32_t*)&Ws[0][0][0] + (4 * v) * 2 + (lane >> 5);
  const unsigned bit = lane & 31;
  double acc[4][MC];
  uint32_t n1[4], n2[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    n1[u] = 0;
    n2[u] = 0;
#pragma unroll
    for (int c = 0; c < MC; ++c) acc[u][c] = 0.0;
  }
  // this thread's share of a tile, fetched while the tile before it is worked on: 4 word pairs
  // (8 per line and homologue) and MC / 4 entries of Y
  u64 gw[4][2];
  double gy[MC / 4];
  auto fetch = [&](int64_t t0) {
    const int tn = (int)min((int64_t)AS_TI, i_end - t0);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int q = tid + 256 * s;
      const int j = q >> 4, hh = (q >> 3) & 1, cq = q & 7;
      gw[s][0] = 0;
      gw[s][1] = 0;
      if (j < tn && wg + 2 * cq < W64) {
        const int64_t lh = (int64_t)rows[t0 + j] * 2 + hh;
        gw[s][0] = G[gnx_word_at(H, lh, wg + 2 * cq)];
        gw[s][1] = G[gnx_word_at(H, lh, wg + 2 * cq + 1)];
      }
    }
#pragma unroll
    for (int s = 0; s < MC / 4; ++s) {
      const int q = tid + 256 * s;
      const int j = q / MC, c = q - j * MC;
      gy[s] = (j < tn && c0 + c < m) ? Yin[(t0 + j) * m + c0 + c] : 0.0;
    }
  };
  if (i_begin < i_end) fetch(i_begin);
  for (int64_t t0 = i_begin; t0 < i_end; t0 += AS_TI) {
    const int tn = (int)min((int64_t)AS_TI, i_end - t0);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int q = tid + 256 * s;
      const int j = q >> 4, hh = (q >> 3) & 1, cq = q & 7;
      Ws[j][hh][2 * cq] = gw[s][0];
      Ws[j][hh][2 * cq + 1] = gw[s][1];
    }
#pragma unroll
    for (int s = 0; s < MC / 4; ++s) {
      const int q = tid + 256 * s;
      Ys[q / MC][q % MC] = gy[s];
    }
    __syncthreads();
    if (t0 + AS_TI < i_end) fetch(t0 + AS_TI);
    for (int j = 0; j < tn; ++j) {
      double y[MC];
#pragma unroll
      for (int c = 0; c < MC; ++c) y[c] = Ys[j][c];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t a = (W32[(j * 2 + 0) * 32 + 2 * u] >> bit) & 1u;
        const uint32_t b = (W32[(j * 2 + 1) * 32 + 2 * u] >> bit) & 1u;
        const uint32_t d = a + b;
        if (INTS) {
          n1[u] += d;
          n2[u] += d >> 1;                              // a & b: d == 2
        }
        const double dd = (double)(int)d;
#pragma unroll
        for (int c = 0; c < MC; ++c) acc[u][c] = fma(dd, y[c], acc[u][c]);
      }
    }
  }
  double* out = P + (int64_t)blockIdx.y * L * m;
  uint32_t* outi = PI + (int64_t)blockIdx.y * L * 2;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t l = (int64_t)(wg + 4 * v + u) * 64 + lane;
    if (l < L) {
#pragma unroll
      for (int c = 0; c < MC; ++c)
        if (c0 + c < m) out[l * m + c0 + c] = acc[u][c];
      if (INTS) {
        outi[l * 2] = n1[u];
        outi[l * 2 + 1] = n2[u];
      }
    }
  }
}

// the stretches added in ascending order: Z [L][m] from P [chunks][L][m]; s1, s2 [L] from the
// counts PI [chunks][L][2] (ones, loci with both bits set)
__global__ void k_assoc_sum(int64_t L, int m, int chunks, const double* __restrict__ P,
                            const uint32_t* __restrict__ PI, double* __restrict__ Z,
                            int64_t* __restrict__ s1, int64_t* __restrict__ s2) {
  const int64_t M = L * m;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < M; t += stride) {
    double s = P[t];
    for (int q = 1; q < chunks; ++q) s += P[(int64_t)q * M + t];
    Z[t] = s;
    if (t < L) {
      int64_t a = 0, b = 0;
      for (int q = 0; q < chunks; ++q) {
        a += PI[((int64_t)q * L + t) * 2];
        b += PI[((int64_t)q * L + t) * 2 + 1];
      }
      s1[t] = a;
      s2[t] = a + 2 * b;
    }
  }
}

namespace {

void assoc_launch(int mc, bool ints, dim3 grid, gnx_state* h, int64_t n, int64_t per, int m,
                  const int32_t* d_rows, const double* d_Y, double* d_P, uint32_t* d_PI) {
#define AS_GO(MC, INTS)                                                                        \
  hipLaunchKernelGGL((k_assoc_cross<MC, INTS>), grid, dim3(256), 0, h->stream, n, per, h->W64, \
                     (int)h->cfg.L, m, d_rows, (const u64*)h->G, gnx_halves(h), d_Y, d_P, d_PI)
  if (mc == 16 && ints) AS_GO(16, true);
  else if (mc == 16) AS_GO(16, false);
  else if (ints) AS_GO(8, true);
  else AS_GO(8, false);
#undef AS_GO
}

}  // namespace

extern "C" int gnx_assoc_cross(gnx_state* h, int64_t n, const int64_t* slots, int32_t m,
                               const double* Y, double* DtY, int64_t* s1, int64_t* s2,
                               int64_t* stretch, int64_t* stretches, double* kernel_ms) {
  const char* who = "gnx_assoc_cross";
  if (stretch) *stretch = 0;
  if (stretches) *stretches = 0;
  if (kernel_ms) *kernel_ms = 0.0;
  GNXCHK(geno_ready(h, who));
  if (m < 1 || m > AS_MMAX) {
    gnx_set_error("%s: 1 <= m <= %d columns (got %d)", who, AS_MMAX, m);
    return 1;
  }
  if (n < 1 || n > (1ll << 30)) {
    gnx_set_error("%s: 1..2^30 individuals (n = %lld)", who, (long long)n);
    return 1;
  }
  if (!Y || !DtY || !s1 || !s2) {
    gnx_set_error("%s: null Y, DtY, s1 or s2", who);
    return 1;
  }
  for (int64_t t = 0; t < n * m; ++t)
    if (!std::isfinite(Y[t])) {
      gnx_set_error("%s: Y is not finite (row %lld, column %lld)", who, (long long)(t / m),
                    (long long)(t % m));
      return 1;
    }
  const int64_t L = h->cfg.L;
  const int lines = (h->W64 + 15) / 16;
  int64_t per = 0;
  int chunks = 0;
  assoc_stretch(n, h->W64, &per, &chunks);
  // 8 or 16 columns per block: the one that pads m with fewer empty columns (16 when equal)
  const int mc = (m + 15) / 16 * 16 <= (m + 7) / 8 * 8 ? 16 : 8;
  const int zc = (m + mc - 1) / mc;

  GnxScratch s(who);
  int32_t* d_rows = nullptr;
  double *d_Y = nullptr, *d_P = nullptr, *d_Z = nullptr;
  uint32_t* d_PI = nullptr;
  int64_t *d_s1 = nullptr, *d_s2 = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows));
  GNXCHK(s.get(&d_Y, (size_t)n * m));
  GNXCHK(s.get(&d_P, (size_t)chunks * L * m));
  GNXCHK(s.get(&d_PI, (size_t)chunks * L * 2));
  GNXCHK(s.get(&d_Z, (size_t)L * m));
  GNXCHK(s.get(&d_s1, (size_t)L));
  GNXCHK(s.get(&d_s2, (size_t)L));
  GNXCHK(gnx_h2d(h, d_Y, Y, (size_t)n * m * sizeof(double)));
  double ms = 0.0;
  int64_t n_launch = 0;
  GnxCallTimer tm(h, &ms, &n_launch);
  tm.start();
  // column chunk 0 also counts the integers; the other chunks run the kernel without them
  assoc_launch(mc, true, dim3(lines, chunks, 1), h, n, per, m, d_rows, d_Y, d_P, d_PI);
  if (zc > 1)
    assoc_launch(mc, false, dim3(lines, chunks, zc - 1), h, n, per, m, d_rows, d_Y, d_P, d_PI);
  hipLaunchKernelGGL(k_assoc_sum, dim3(gnx_grid(L * m, 256, 256 * 64)), dim3(256), 0, h->stream,
                     L, m, chunks, d_P, d_PI, d_Z, d_s1, d_s2);
  HIPCHK(hipGetLastError());
  GNXCHK(tm.stop(zc > 1 ? 3 : 2));
  if (stretch) *stretch = per;
  if (stretches) *stretches = chunks;
  if (kernel_ms) *kernel_ms = ms;
  GNXCHK(gnx_d2h(h, DtY, d_Z, (size_t)L * m * sizeof(double)));
  GNXCHK(gnx_d2h(h, s1, d_s1, (size_t)L * sizeof(int64_t)));
  return gnx_d2h(h, s2, d_s2, (size_t)L * sizeof(int64_t));
}
