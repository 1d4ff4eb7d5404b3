// Genetic PCA and genetic distances on the device (reference sim/model.py:2031-2041,
// plot_genetic_PCA; demos/_IBD_IBE.py:38-192, calc_dists): products with the dosage matrix
// D (d = a + b in {0, 1, 2}, a and b the bits of homologues 0 and 1) read straight from the
// bit-packed genome table through the block table, without ever downloading N x L.
//
//   gnx_geno_gram     G = D_S D_S^T, exact int64, n <= 8192      (popcounts, 64 x 64 LDS tiles)
//   gnx_geno_matmul   Y = D_S M,   M [L][k] fp32, k <= 64        (thread = individual)
//   gnx_geno_rmatmul  Z = D_S^T Y, Y [n][k] fp32                 (lane = locus)
//
// The products use plain fp32 FMAs: d * m is exact, so each output is an fp32 sum of exact
// products and meets the any-order bound of DESIGN.md (and is exact for integer inputs whose
// absolute sums stay below 2^24).  Rows follow the order of the slots given.
#include "gnx_geno.h"

__global__ void k_geno_rows(int64_t n, const int64_t* __restrict__ slots,
                            const int32_t* __restrict__ grow, int32_t* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) rows[i] = grow[slots ? slots[i] : i];
}

// ---------------------------------------------------------------- Gram
// X[i][hom][q] = word widx[q] of row i's homologue, masked (q >= nw and i >= n: 0)
__global__ void k_geno_gather(int64_t n, int64_t n_pad, int nw, int Wm,
                              const int32_t* __restrict__ rows, const int32_t* __restrict__ widx,
                              const u64* __restrict__ wmask, const u64* __restrict__ G, GnxHalves H,
                              u64* __restrict__ X) {
  const int64_t total = n_pad * 2 * Wm;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t i = t / (2 * Wm);
    const int r = (int)(t - i * 2 * Wm);
    const int hh = r >= Wm ? 1 : 0;
    const int q = r - hh * Wm;
    u64 v = 0;
    if (i < n && q < nw) v = G[gnx_word_at(H, (int64_t)rows[i] * 2 + hh, widx[q])] & wmask[q];
    X[t] = v;
  }
}

// one 64 x 64 tile of G per block (upper triangle of tiles only, mirrored on the write);
// thread (tx, ty) owns rows ty + 16 r and columns tx + 16 c.  LDS: [word][hom][row], 16 words
// per stage, so consecutive threads read consecutive u64.
__global__ void __launch_bounds__(256)
k_geno_gram(int64_t n, int Wm, const u64* __restrict__ X, int64_t* __restrict__ out) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj < ti) return;                              // block-uniform
  __shared__ u64 As[GRAM_GK][2][64];
  __shared__ u64 Bs[GRAM_GK][2][64];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t i0 = (int64_t)ti * 64, j0 = (int64_t)tj * 64;
  int acc[4][4] = {};
  for (int k0 = 0; k0 < Wm; k0 += GRAM_GK) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int q = tid + 256 * s;                    // (row, hom, word) with the word fastest
      const int row = q >> 5, hh = (q >> 4) & 1, kk = q & 15;
      As[kk][hh][row] = X[((i0 + row) * 2 + hh) * Wm + k0 + kk];
      Bs[kk][hh][row] = X[((j0 + row) * 2 + hh) * Wm + k0 + kk];
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < GRAM_GK; ++kk) {
      u64 ai[4], bi[4], aj[4], bj[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ai[r] = As[kk][0][ty + 16 * r];
        bi[r] = As[kk][1][ty + 16 * r];
        aj[r] = Bs[kk][0][tx + 16 * r];
        bj[r] = Bs[kk][1][tx + 16 * r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[r][c] += __popcll(ai[r] & aj[c]) + __popcll(ai[r] & bj[c]) +
                       __popcll(bi[r] & aj[c]) + __popcll(bi[r] & bj[c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
      if (i < n && j < n) {
        out[i * n + j] = acc[r][c];
        out[j * n + i] = acc[r][c];
      }
    }
}

extern "C" int gnx_geno_gram(gnx_state* h, int64_t n, const int64_t* slots,
                             const uint64_t* locus_mask, int64_t* Gout) {
  const char* who = "gnx_geno_gram";
  GNXCHK(geno_ready(h, who));
  if (n < 1 || n > 8192) {
    gnx_set_error("%s: 1..8192 individuals per call (the matrix is n x n)", who);
    return 1;
  }
  if (!Gout) {
    gnx_set_error("%s: null output", who);
    return 1;
  }
  GnxScratch s(who);
  int32_t* d_rows = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows));
  int64_t* d_out = nullptr;
  GNXCHK(geno_gram_dev(h, s, d_rows, n, locus_mask, &d_out));
  HIPCHK(hipGetLastError());
  return gnx_d2h(h, Gout, d_out, (size_t)n * n * sizeof(int64_t));
}

// ---------------------------------------------------------------- Y = D M
// Thread = individual, GENO_KC = 16 columns per block (blockIdx.y: the column chunk).  A stage
// of MM_WS words (512 loci) of M sits in LDS and every lane reads the same entry (a broadcast);
// the lane's own words come straight from the genome table.  Rows of M past L read as 0, so
// the padding bits past L add nothing.
#define GENO_KC 16
#define MM_WS 8
__global__ void __launch_bounds__(256)
k_geno_matmul(int64_t n, int W64, int L, int k, const int32_t* __restrict__ rows,
              const u64* __restrict__ G, GnxHalves H, const float* __restrict__ M,
              float* __restrict__ Y) {
  __shared__ float Ms[MM_WS * 64][GENO_KC];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c0 = blockIdx.y * GENO_KC;
  const bool live = i < n;
  const int64_t lh = live ? (int64_t)rows[i] * 2 : 0;
  float acc[GENO_KC];
#pragma unroll
  for (int c = 0; c < GENO_KC; ++c) acc[c] = 0.f;
  for (int w0 = 0; w0 < W64; w0 += MM_WS) {
    __syncthreads();
    for (int q = threadIdx.x; q < MM_WS * 64 * GENO_KC; q += 256) {
      const int r = q / GENO_KC, c = q - r * GENO_KC;
      const int64_t l = (int64_t)w0 * 64 + r;
      Ms[r][c] = (l < L && c0 + c < k) ? M[l * k + c0 + c] : 0.f;
    }
    __syncthreads();
    if (!live) continue;
    for (int u = 0; u < MM_WS && w0 + u < W64; ++u) {
      const u64 a = G[gnx_word_at(H, lh, w0 + u)];
      const u64 b = G[gnx_word_at(H, lh + 1, w0 + u)];
      if ((a | b) == 0ull) continue;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const unsigned int ah = (unsigned int)(a >> (32 * half));
        const unsigned int bh = (unsigned int)(b >> (32 * half));
#pragma unroll 4
        for (int bit = 0; bit < 32; ++bit) {
          const float d = (float)(((ah >> bit) & 1u) + ((bh >> bit) & 1u));
          const float* m = Ms[u * 64 + half * 32 + bit];
#pragma unroll
          for (int c = 0; c < GENO_KC; ++c) acc[c] = __fmaf_rn(d, m[c], acc[c]);
        }
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int c = 0; c < GENO_KC; ++c)
    if (c0 + c < k) Y[i * k + c0 + c] = acc[c];
}

extern "C" int gnx_geno_matmul(gnx_state* h, int32_t k, const float* M, float* Y, int64_t n,
                               const int64_t* slots) {
  const char* who = "gnx_geno_matmul";
  GNXCHK(geno_ready(h, who));
  if (k < 1 || k > 64 || n < 0 || !M || (!Y && n > 0)) {
    gnx_set_error("%s: 1 <= k <= 64, n >= 0 and device pointers M, Y", who);
    return 1;
  }
  GnxScratch s(who);
  int32_t* d_rows = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows));
  if (n > 0)
    hipLaunchKernelGGL(k_geno_matmul,
                       dim3((unsigned)((n + 255) / 256), (k + GENO_KC - 1) / GENO_KC), dim3(256),
                       0, h->stream, n, h->W64, h->cfg.L, k, d_rows, (const u64*)h->G,
                       gnx_halves(h), M, Y);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// ---------------------------------------------------------------- Z = D^T Y
// Block = one 128-byte line of the genome (16 words, 1024 loci): wave v owns words 4v..4v+3,
// lane = locus within the word, so every (locus, column) of the block has exactly one owner.
// Tiles of RM_TI individuals are staged in LDS (their 16 words per homologue, and their rows
// of Y); every lane reads the same entries (broadcasts).  blockIdx.y = a stretch of
// individuals whose partial sums go to P[chunk][L][k]; blockIdx.z = the column chunk.  A
// second kernel adds the chunks in a fixed order, so the result does not depend on scheduling.
#define RM_TI 128
__global__ void __launch_bounds__(256)
k_geno_rmatmul(int64_t n, int64_t per_chunk, int W64, int L, int k,
               const int32_t* __restrict__ rows, const u64* __restrict__ G, GnxHalves H,
               const float* __restrict__ Yin, float* __restrict__ P) {
  __shared__ u64 Ws[RM_TI][2][16];
  __shared__ float Ys[RM_TI][GENO_KC];
  const int tid = threadIdx.x, lane = tid & 63, v = tid >> 6;
  const int wg = blockIdx.x * 16;                       // first word of the block's line
  const int c0 = blockIdx.z * GENO_KC;
  const int64_t i_begin = (int64_t)blockIdx.y * per_chunk;
  const int64_t i_end = min(n, i_begin + per_chunk);
  float acc[4][GENO_KC];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int c = 0; c < GENO_KC; ++c) acc[u][c] = 0.f;
  for (int64_t t0 = i_begin; t0 < i_end; t0 += RM_TI) {
    const int tn = (int)min((int64_t)RM_TI, i_end - t0);
    __syncthreads();
    for (int q = tid; q < RM_TI * 2 * 8; q += 256) {      // word pairs, 8 per line
      const int j = q >> 4, hh = (q >> 3) & 1, cq = q & 7;
      u64 x0 = 0, x1 = 0;
      if (j < tn && wg + 2 * cq < W64) {
        const int64_t lh = (int64_t)rows[t0 + j] * 2 + hh;
        x0 = G[gnx_word_at(H, lh, wg + 2 * cq)];
        x1 = G[gnx_word_at(H, lh, wg + 2 * cq + 1)];
      }
      Ws[j][hh][2 * cq] = x0;
      Ws[j][hh][2 * cq + 1] = x1;
    }
    for (int q = tid; q < RM_TI * GENO_KC; q += 256) {
      const int j = q / GENO_KC, c = q - j * GENO_KC;
      Ys[j][c] = (j < tn && c0 + c < k) ? Yin[(t0 + j) * k + c0 + c] : 0.f;
    }
    __syncthreads();
    for (int j = 0; j < tn; ++j) {
      float y[GENO_KC];
#pragma unroll
      for (int c = 0; c < GENO_KC; ++c) y[c] = Ys[j][c];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const u64 a = Ws[j][0][4 * v + u], b = Ws[j][1][4 * v + u];
        const float d = (float)((int)((a >> lane) & 1ull) + (int)((b >> lane) & 1ull));
#pragma unroll
        for (int c = 0; c < GENO_KC; ++c) acc[u][c] = __fmaf_rn(d, y[c], acc[u][c]);
      }
    }
  }
  float* out = P + (int64_t)blockIdx.y * L * k;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t l = (int64_t)(wg + 4 * v + u) * 64 + lane;
    if (l < L) {
#pragma unroll
      for (int c = 0; c < GENO_KC; ++c)
        if (c0 + c < k) out[l * k + c0 + c] = acc[u][c];
    }
  }
}

__global__ void k_geno_chunk_sum(int64_t m, int chunks, const float* __restrict__ P,
                                 float* __restrict__ Z) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += stride) {
    float s = P[t];
    for (int q = 1; q < chunks; ++q) s += P[(int64_t)q * m + t];
    Z[t] = s;
  }
}

extern "C" int gnx_geno_rmatmul(gnx_state* h, int32_t k, const float* Y, float* Z, int64_t n,
                                const int64_t* slots) {
  const char* who = "gnx_geno_rmatmul";
  GNXCHK(geno_ready(h, who));
  if (k < 1 || k > 64 || n < 0 || !Z || (!Y && n > 0)) {
    gnx_set_error("%s: 1 <= k <= 64, n >= 0 and device pointers Y, Z", who);
    return 1;
  }
  GnxScratch s(who);
  int32_t* d_rows = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows));
  const int L = h->cfg.L;
  const int lines = (h->W64 + 15) / 16;
  // enough blocks to fill the device (~2048), each stretch at least one tile of individuals
  const int64_t tiles = std::max<int64_t>(1, (n + RM_TI - 1) / RM_TI);
  const int chunks = (int)std::min<int64_t>(std::min<int64_t>(tiles, 32),
                                            std::max(1, 2048 / lines));
  const int64_t per_chunk = (tiles + chunks - 1) / chunks * RM_TI;
  const int64_t m = (int64_t)L * k;
  float* P = Z;
  if (chunks > 1) GNXCHK(s.get(&P, (size_t)chunks * m));
  hipLaunchKernelGGL(k_geno_rmatmul, dim3(lines, chunks, (k + GENO_KC - 1) / GENO_KC), dim3(256),
                     0, h->stream, n, per_chunk, h->W64, L, k, d_rows, (const u64*)h->G,
                     gnx_halves(h), Y, P);
  if (chunks > 1)
    hipLaunchKernelGGL(k_geno_chunk_sum, dim3(gnx_grid(m, 256, 256 * 64)), dim3(256), 0,
                       h->stream, m, chunks, P, Z);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}
