// Weighted genomic relationship matrices on the device (gnx_grm, include/gnx_hip.h): the
// symmetric rank-L update G_ij = sum_l val[l][d_il] val[l][d_jl] over the loci of a mask, d the
// dosage of the sampled individuals, val a host-written table of three fp32 values per locus.
// One table form covers the additive GRM in any weighting (GCTA, VanRaden, the alpha model),
// the dominance GRM and LD-weighted GRMs (geonomics_amd/sim/quantgen.py writes them); a real
// weight per locus is what the popcounts of gnx_geno_gram cannot carry.
//
//   gnx_grm        G [n][n] fp64, n <= 8192            (f32 MFMA, 128 x 128 LDS tiles)
//   gnx_grm_info   tiles, fp32 chains per entry and kernel time of the last call
//   gnx_grm_probe  a measuring switch: time the expansion or the MFMAs alone (no result)
//
// The operand is the gathered X [rows][2][words] of the Gram kernel (gnx_geno.h: masked words
// only, rows past n zero).  One 128 x 128 tile of G per 256-thread block, upper triangle of tiles
// only, mirrored on the write; the waves' share of it, the MFMA loop and the numerics contract
// are MmWave's (gnx_mfma.h).  A stage is MM_KS = 32 loci (half a word): thread t expands the 32
// bits of row t & 127 of the tile's rows (t < 128) or columns (t >= 128) to fp32 - two bit
// extracts, an add, and one LDS read of the word's table at [locus][d] - into S[op][locus][row],
// once per block, and all four waves read their MFMA operands from there.
//
// Numerics (gnx_mfma.h).  The chains are flushed after GRM_FLUSH = 16 words (at most 1024 used
// loci); the fp64 sum runs in word order.  The mirror writes the value itself, and a diagonal
// tile writes only its upper triangle (and mirrors it), so G == G^T exactly.
#include "gnx_geno.h"
#include "gnx_mfma.h"

#define GRM_FLUSH 16     // words per fp32 chain: 1024 loci

// tab [nw][64][4]: the word's table, entry [bit][d] for d = 0, 1, 2 and [bit][3] = 0.
// MODE 0 is the kernel; 1 (the expansion alone, no MFMA) and 2 (the MFMAs alone, on a stage of
// zeros) only split its time for tools/grm_bench.py (gnx_grm_probe): zeros come back.
template <int MODE>
// two blocks per CU (225 VGPRs, 34 KiB of LDS): one block's expansion runs under the other's MFMAs
__global__ void __launch_bounds__(256, 2)
k_grm(int64_t n, int nw, int Wm, const u64* __restrict__ X, const float* __restrict__ tab,
      double* __restrict__ out) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj < ti) return;                              // block-uniform
  __shared__ float S[2][MM_KS][MM_T];
  __shared__ float vt[2][64 * 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t i0 = (int64_t)ti * MM_T, j0 = (int64_t)tj * MM_T;
  // the expansion's share of this thread: one row of the rows (op 0) or columns (op 1)
  const int op = tid >> 7, xrow = tid & (MM_T - 1);
  const int64_t gi = (op ? j0 : i0) + xrow;
  const unsigned dead = gi < n ? 0u : 3u;
  const u64* xa = X + (gi * 2) * Wm;
  const u64* xb = xa + Wm;
  float* dst = &S[op][0][xrow];
  const float* sa = mm_operand(S[0], wr * 64, lane);
  const float* sb = mm_operand(S[1], wc * 64, lane);

  MmWave W;
  W.clear();

  if (MODE == 2) {
    for (int q = tid; q < 2 * MM_KS * MM_T; q += 256) (&S[0][0][0])[q] = 0.f;
  }
  u64 a = 0, b = 0;
  float tv = 0.f;
  if (nw > 0) {
    a = xa[0];
    b = xb[0];
    tv = tab[tid];
  }
  for (int q = 0; q < nw; ++q) {
    const int p = q & 1;
    vt[p][tid] = tv;                      // read last two words ago: two barriers in between
    const u64 ca = a, cb = b;
    if (q + 1 < nw) {                     // the next word's, in flight under this word's MFMAs
      a = xa[q + 1];
      b = xb[q + 1];
      tv = tab[(int64_t)(q + 1) * 256 + tid];
    }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      __syncthreads();                    // the last stage's operands are read; vt[p] is written
      const unsigned a32 = (unsigned)(ca >> (32 * hf)), b32 = (unsigned)(cb >> (32 * hf));
      const float* t = &vt[p][hf * MM_KS * 4];
      if (MODE != 2) {
#pragma unroll
        for (int l = 0; l < MM_KS; ++l) dst[l * MM_T] = mm_dosage(t, a32, b32, l, dead);
      }
      __syncthreads();
      if (MODE == 1) continue;
      W.stage(sa, sb);
    }
    if ((q + 1) % GRM_FLUSH == 0 || q + 1 == nw) W.flush();      // block-uniform
  }
  if (MODE == 1) return;               // (MODE 2 writes its zeros: the MFMAs must stay live)
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int64_t i = mm_row(i0 + wr * 64 + m * 32, e, lane);
        const int64_t j = j0 + wc * 64 + c * 32 + (lane & 31);
        if (i < n && j < n && (ti != tj || j >= i)) {
          out[i * n + j] = W.sum[m][c][e];
          if (i != j) out[j * n + i] = W.sum[m][c][e];
        }
      }
}

extern "C" int gnx_grm_probe(gnx_state* h, int32_t mode) {
  if (mode < 0 || mode > 2) {
    gnx_set_error("gnx_grm_probe: mode 0 (the kernel), 1 (expansion alone) or 2 (MFMAs alone)");
    return 1;
  }
  h->grm_probe = mode;
  return 0;
}

extern "C" int gnx_grm_info(gnx_state* h, int64_t* tiles, int64_t* k_chunks, double* kernel_ms) {
  if (tiles) *tiles = h->grm_tiles;
  if (k_chunks) *k_chunks = h->grm_chunks;
  if (kernel_ms) *kernel_ms = h->grm_ms;
  return 0;
}

extern "C" int gnx_grm(gnx_state* h, int64_t n, const int64_t* slots, const uint64_t* locus_mask,
                       const float* val, double* Gout) {
  const char* who = "gnx_grm";
  GNXCHK(geno_ready(h, who));
  if (n < 1 || n > 8192) {
    gnx_set_error("%s: 1..8192 individuals per call (the matrix is n x n)", who);
    return 1;
  }
  if (!val || !Gout) {
    gnx_set_error("%s: null table or output", who);
    return 1;
  }
  h->grm_ms = 0.0;
  h->grm_launches = h->grm_tiles = h->grm_chunks = 0;
  GnxScratch s(who);
  int32_t* d_rows = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows));
  std::vector<int32_t> widx;
  std::vector<u64> wmask;
  geno_words(h, locus_mask, widx, wmask);
  const int64_t n_pad = (n + MM_T - 1) / MM_T * MM_T;
  const int T = (int)(n_pad / MM_T);
  GenoOperand op;
  GNXCHK(geno_operand(h, s, n_pad, widx, wmask, 0, &op));
  const std::vector<float> tab = geno_tables(op, widx, wmask, val, op.nw);
  float* d_tab = nullptr;
  double* d_G = nullptr;
  GNXCHK(s.get(&d_tab, tab.size()));
  GNXCHK(s.get(&d_G, (size_t)n * n));
  if (!tab.empty()) GNXCHK(gnx_h2d(h, d_tab, tab.data(), tab.size() * sizeof(float)));
  GnxCallTimer tm(h, &h->grm_ms, &h->grm_launches);
  tm.start();
  geno_gather(h, d_rows, n, op);
  auto* kern = h->grm_probe == 1 ? k_grm<1> : h->grm_probe == 2 ? k_grm<2> : k_grm<0>;
  if (h->grm_probe) HIPCHK(hipMemsetAsync(d_G, 0, (size_t)n * n * sizeof(double), h->stream));
  hipLaunchKernelGGL(kern, dim3(T, T), dim3(256), 0, h->stream, n, op.nw, op.Wm,
                     (const u64*)op.X, (const float*)d_tab, d_G);
  HIPCHK(hipGetLastError());
  GNXCHK(tm.stop(2));
  h->grm_tiles = (int64_t)T * (T + 1) / 2;
  h->grm_chunks = (op.nw + GRM_FLUSH - 1) / GRM_FLUSH;
  return gnx_d2h(h, Gout, d_G, (size_t)n * n * sizeof(double));
}
