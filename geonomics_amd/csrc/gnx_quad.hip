// Per-locus quadratic forms on the device (gnx_assoc_quad, include/gnx_hip.h):
//   q[l] = sum over k < m of ( sum over i < n of M[k][i] val[l][d_il] )^2,
// d the dosage of the sampled individuals, val the three-value table of gnx_grm (the host writes
// the centring into it), M a host matrix fp32 [m][n].  With M = diag((lambda + delta)^-1/2) U^T
// of a relationship matrix this is z_l^T (G + delta I)^-1 z_l, the one term of the mixed-model
// association scan (geonomics_amd/sim/assoc.py, lmm_*) that costs 2 n m L FLOP; with the top
// eigenvectors alone it is the communality of every locus.  Nothing n x L or m x L is written.
//
// The operand is the gathered X [rows][2][words] of the Gram kernel (gnx_geno.h: masked words
// only, rows past n zero).  One 256-thread block per 128 rows of M x 128 loci (two words of the
// list) of C = M Z; the waves' share of it, the MFMA loop and the numerics contract are MmWave's
// (gnx_mfma.h).  The reduction runs over the individuals in stages of MM_KS = 32.  Per stage
// thread (ind = t >> 3, seg = t & 7) copies 16 floats of row i0 + ind of M^T (k_quad_transpose
// writes it first, padded with zero rows to a multiple of 32 and zero columns to a multiple of
// 128, so the copy is contiguous along k) and expands 16 loci of individual i0 + ind through the
// block's table, which sits in LDS once per block: a block's loci do not change.  The next stage's 16 floats and two words are loaded before the
// MFMAs of the current one.  The locus tile is the fastest grid dimension: consecutive blocks
// read the same 128 x n slab of M (4 MiB at n = 8192) out of L2.
//
// Numerics (gnx_mfma.h).  The chains are flushed after QD_FLUSH = 32 stages (1024 individuals):
//   |dC_kl| <= e_kl := (1.01 min(n, 1024) 2^-24 + n 2^-53) sum_i |M_ki z_il|,
//   |dq_l|  <= sum_k (2 |C_kl| e_kl + e_kl^2) + m 2^-53 q_l.
// The epilogue has one order and no atomics: a lane squares its fp64 sums and adds them over the
// 16 elements and the two row accumulators in index order, adds its lane ^ 32 partner, the two
// wr waves meet in LDS, and one partial per (128 rows of M, locus) is written; k_quad_sum adds
// the partials in ascending row order.  A repeated call is bit-equal.
//
// The padding rows and columns of M^T are zero, so they too contribute exactly 0.
#include <cmath>
#include <cstring>
#include "gnx_geno.h"
#include "gnx_mfma.h"

#define QD_FLUSH 32      // stages per fp32 chain: 1024 individuals
#define QD_VT 68         // floats of the table per 16 loci: 64 and 4 of padding (LDS banks)

// Mt [n_pad][m_pad] = M^T padded; X [n_pad][2][Wm]; tab [nwp][64][4] with [bit][3] = 0;
// P [m_pad / 128][nwp * 64]: P[kt][c] = sum over the rows k of tile kt of C_kc^2
// two blocks per CU: one block's copies and expansion run under the other's MFMAs
__global__ void __launch_bounds__(256, 2)
k_quad(int64_t n, int64_t n_pad, int64_t m_pad, int Wm, int64_t Lp, const float* __restrict__ Mt,
       const u64* __restrict__ X, const float* __restrict__ tab, double* __restrict__ P) {
  // [0]: M^T slab [i][k], [1]: Z [i][locus]; written as float4
  __shared__ __attribute__((aligned(16))) float S[2][MM_KS][MM_T];
  __shared__ float vt[8 * QD_VT];
  __shared__ double red[2][MM_T];
  const int lt = blockIdx.x, kt = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, r = lane & 31, hk = lane >> 5;
  const int ind = tid >> 3, seg = tid & 7;
  const float* ma = Mt + (int64_t)ind * m_pad + (int64_t)kt * MM_T + seg * 16;
  const u64* xa = X + ((int64_t)ind * 2) * Wm + lt * 2 + (seg >> 2);
  const int sh = (seg & 3) * 16;
  float4* da = reinterpret_cast<float4*>(&S[0][ind][seg * 16]);
  float4* db = reinterpret_cast<float4*>(&S[1][ind][seg * 16]);
  const float* t = &vt[seg * QD_VT];
  const float* sa = mm_operand(S[0], wr * 64, lane);
  const float* sb = mm_operand(S[1], wc * 64, lane);

  for (int j = tid; j < MM_T * 4; j += 256)    // locus j >> 2 of the tile, entry j & 3
    vt[(j >> 6) * QD_VT + (j & 63)] = tab[(int64_t)lt * (MM_T * 4) + j];

  MmWave W;
  W.clear();

  const int stages = (int)(n_pad / MM_KS);
  const float4* m4 = reinterpret_cast<const float4*>(ma);
  float4 p0 = m4[0], p1 = m4[1], p2 = m4[2], p3 = m4[3];
  u64 ha = xa[0], hb = xa[Wm];
  for (int s = 0; s < stages; ++s) {
    const unsigned a16 = (unsigned)(ha >> sh) & 0xffffu, b16 = (unsigned)(hb >> sh) & 0xffffu;
    const unsigned dead = s * MM_KS + ind < (int)n ? 0u : 3u;
    __syncthreads();                      // the last stage's operands are read; vt is written
    da[0] = p0;
    da[1] = p1;
    da[2] = p2;
    da[3] = p3;
    auto z = [&](int l) { return mm_dosage(t, a16, b16, l, dead); };
    db[0] = make_float4(z(0), z(1), z(2), z(3));
    db[1] = make_float4(z(4), z(5), z(6), z(7));
    db[2] = make_float4(z(8), z(9), z(10), z(11));
    db[3] = make_float4(z(12), z(13), z(14), z(15));
    if (s + 1 < stages) {                 // the next stage's, in flight under this stage's MFMAs
      ma += MM_KS * m_pad;
      xa += (int64_t)MM_KS * 2 * Wm;
      m4 = reinterpret_cast<const float4*>(ma);
      p0 = m4[0];
      p1 = m4[1];
      p2 = m4[2];
      p3 = m4[3];
      ha = xa[0];
      hb = xa[Wm];
    }
    __syncthreads();
    W.stage(sa, sb);
    if ((s + 1) % QD_FLUSH == 0 || s + 1 == stages) W.flush();   // block-uniform
  }
  // C/D of the 32 x 32 MFMA: column = lane & 31; a lane's 16 elements and its lane ^ 32 partner's
  // are the 32 rows of that column, and every row of M is summed: the row map does not matter
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    double v = 0.0;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int e = 0; e < 16; ++e) v += W.sum[mi][c][e] * W.sum[mi][c][e];
    v += __shfl_xor(v, 32);
    if (hk == 0) red[wr][wc * 64 + c * 32 + r] = v;
  }
  __syncthreads();
  if (tid < MM_T) P[(int64_t)kt * Lp + (int64_t)lt * MM_T + tid] = red[0][tid] + red[1][tid];
}

// Mt[i][k] = M[k][i] for k < m, i < n, in 32 x 32 tiles through LDS (block 32 x 8); the padding
// of Mt [n_pad][m_pad] is zeroed by the caller
__global__ void k_quad_transpose(int m, int n, int64_t m_pad, const float* __restrict__ M,
                                 float* __restrict__ Mt) {
  __shared__ float tile[32][33];
  const int i0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
  for (int r = threadIdx.y; r < 32; r += 8) {
    const int k = k0 + r, i = i0 + threadIdx.x;
    if (k < m && i < n) tile[r][threadIdx.x] = M[(int64_t)k * n + i];
  }
  __syncthreads();
  for (int r = threadIdx.y; r < 32; r += 8) {
    const int i = i0 + r, k = k0 + threadIdx.x;
    if (i < n && k < m) Mt[(int64_t)i * m_pad + k] = tile[threadIdx.x][r];
  }
}

// q[locus of (word j >> 6 of the list, bit j & 63)] = the partials of the row tiles, ascending
__global__ void k_quad_sum(int64_t nbits, int KT, int64_t Lp, const int32_t* __restrict__ widx,
                           const u64* __restrict__ wmask, const double* __restrict__ P,
                           double* __restrict__ q) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nbits) return;
  const int w = (int)(j >> 6), bit = (int)(j & 63);
  if (!((wmask[w] >> bit) & 1ull)) return;
  double v = 0.0;
  for (int kt = 0; kt < KT; ++kt) v += P[(int64_t)kt * Lp + j];
  q[(int64_t)widx[w] * 64 + bit] = v;
}

namespace {

// the index of the first NaN or infinity of p [cnt], or -1: whole blocks are tested without a
// branch (the loop vectorises; M is 64 M floats at n = m = 8192)
int64_t quad_first_nonfinite(const float* p, int64_t cnt) {
  const int64_t B = 4096;
  for (int64_t a = 0; a < cnt; a += B) {
    const int64_t e = std::min(cnt, a + B);
    uint32_t bad = 0;
    for (int64_t t = a; t < e; ++t) {
      uint32_t u;
      memcpy(&u, p + t, sizeof u);
      bad |= (uint32_t)((u & 0x7f800000u) == 0x7f800000u);
    }
    if (bad)
      for (int64_t t = a; t < e; ++t)
        if (!std::isfinite(p[t])) return t;
  }
  return -1;
}

}  // namespace

extern "C" int gnx_assoc_quad(gnx_state* h, int64_t n, const int64_t* slots,
                              const uint64_t* locus_mask, const float* val, int32_t m,
                              const float* M, double* q, double* kernel_ms) {
  const char* who = "gnx_assoc_quad";
  if (kernel_ms) *kernel_ms = 0.0;
  GNXCHK(geno_ready(h, who));
  if (n < 1 || n > 8192) {
    gnx_set_error("%s: 1..8192 individuals per call (M is m x n)", who);
    return 1;
  }
  if (m < 1 || m > 8192) {
    gnx_set_error("%s: 1 <= m <= 8192 rows of M (got %d)", who, m);
    return 1;
  }
  if (!val || !M || !q) {
    gnx_set_error("%s: null table, M or output", who);
    return 1;
  }
  const int64_t L = h->cfg.L;
  int64_t t = quad_first_nonfinite(val, L * 3);
  if (t >= 0) {
    gnx_set_error("%s: val is not finite (locus %lld)", who, (long long)(t / 3));
    return 1;
  }
  t = quad_first_nonfinite(M, (int64_t)m * n);
  if (t >= 0) {
    gnx_set_error("%s: M is not finite (row %lld, column %lld)", who, (long long)(t / n),
                  (long long)(t % n));
    return 1;
  }
  GnxScratch s(who);
  int32_t* d_rows = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows));
  std::fill(q, q + L, 0.0);
  std::vector<int32_t> widx;
  std::vector<u64> wmask;
  geno_words(h, locus_mask, widx, wmask);
  if (widx.empty()) return 0;
  const int64_t n_pad = (n + MM_KS - 1) / MM_KS * MM_KS;
  const int64_t m_pad = ((int64_t)m + MM_T - 1) / MM_T * MM_T;
  const int KT = (int)(m_pad / MM_T);
  GenoOperand op;
  GNXCHK(geno_operand(h, s, n_pad, widx, wmask, 0, &op));
  const int nwp = (op.nw + 1) / 2 * 2;          // whole locus tiles; nwp <= Wm, a multiple of 16
  const int LT = nwp / 2;
  const int64_t Lp = (int64_t)nwp * 64;
  const std::vector<float> tab = geno_tables(op, widx, wmask, val, nwp);
  float *d_tab = nullptr, *d_M = nullptr, *d_Mt = nullptr;
  double *d_P = nullptr, *d_q = nullptr;
  GNXCHK(s.get(&d_tab, tab.size()));
  GNXCHK(s.get(&d_M, (size_t)m * n));
  GNXCHK(s.get(&d_Mt, (size_t)n_pad * m_pad));
  GNXCHK(s.get(&d_P, (size_t)KT * Lp));
  GNXCHK(s.get(&d_q, (size_t)h->W64 * 64));
  GNXCHK(gnx_h2d(h, d_tab, tab.data(), tab.size() * sizeof(float)));
  GNXCHK(gnx_h2d(h, d_M, M, (size_t)m * n * sizeof(float)));
  double ms = 0.0;
  int64_t n_launch = 0;
  GnxCallTimer tm(h, &ms, &n_launch);
  tm.start();
  HIPCHK(hipMemsetAsync(d_q, 0, (size_t)h->W64 * 64 * sizeof(double), h->stream));
  // M^T with zero padding, transposed on the device: on the host the strided copy of 8192 x 8192
  // floats into a second 256 MiB buffer took 0.3 s per call, beside 13 ms of kernels at L = 10^4
  HIPCHK(hipMemsetAsync(d_Mt, 0, (size_t)n_pad * m_pad * sizeof(float), h->stream));
  hipLaunchKernelGGL(k_quad_transpose, dim3((unsigned)((n + 31) / 32), (unsigned)((m + 31) / 32)),
                     dim3(32, 8), 0, h->stream, (int)m, (int)n, m_pad, (const float*)d_M, d_Mt);
  geno_gather(h, d_rows, n, op);
  hipLaunchKernelGGL(k_quad, dim3(LT, KT), dim3(256), 0, h->stream, n, n_pad, m_pad, op.Wm, Lp,
                     (const float*)d_Mt, (const u64*)op.X, (const float*)d_tab, d_P);
  const int64_t nbits = (int64_t)op.nw * 64;
  hipLaunchKernelGGL(k_quad_sum, dim3(gnx_grid(nbits, 256)), dim3(256), 0, h->stream, nbits, KT,
                     Lp, (const int32_t*)op.widx, (const u64*)op.wmask, (const double*)d_P, d_q);
  HIPCHK(hipGetLastError());
  GNXCHK(tm.stop(4));
  if (kernel_ms) *kernel_ms = ms;
  return gnx_d2h(h, q, d_q, (size_t)L * sizeof(double));
}
