// What the entry points that read the dosage matrix share (gnx_geno.hip: products over the
// individuals; gnx_gea.hip: cross-products over the loci; gnx_mantel.hip: distance cross-sums
// under permutation; gnx_sgs.hip, gnx_ld.hip, gnx_tracts.hip: pair statistics): the
// preconditions, the slots' genome rows, the masked word list, the gathered operand
// X [rows][2][words] of the 64 x 64 tile kernels, and the popcount Gram matrix on the device.
// (The call's device scratch, GnxScratch, is in gnx_internal.h.)
#pragma once
#include <algorithm>
#include <vector>
#include "gnx_internal.h"

typedef unsigned long long u64;

// words per LDS stage of the 64 x 64 tile: the word count of its operand is a multiple of it
#define GRAM_GK 16

// ---- the 64 x 64 popcount tile of a 256-thread block over X [rows][2][Wm] (k_sgs_pairs,
// k_tract_pairs).  LDS: [word][hom][row], GRAM_GK words of the tile's 64 rows (A) and 64
// columns (B) per stage, so consecutive threads read consecutive u64.  The kernel declares the
// stage __shared__.  (k_geno_gram and kin_tile of gnx_kin.hip keep their own copies of the
// walk: the two kernels with one tile per block measured 1 to 5 % slower on geno_tile64, the
// two that stride over a task list did not)
struct GenoStage {
  u64 A[GRAM_GK][2][64];
  u64 B[GRAM_GK][2][64];
};

// words k0 .. k0 + GRAM_GK - 1 of rows a0 .. a0 + 63 into S.A and of rows b0 .. b0 + 63 into S.B
// (no barrier: the caller places them)
__device__ __forceinline__ void geno_stage_load(GenoStage& S, const u64* __restrict__ X, int Wm,
                                                int64_t a0, int64_t b0, int k0) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int q = tid + 256 * s;                      // (row, hom, word) with the word fastest
    const int row = q >> 5, hh = (q >> 4) & 1, kk = q & 15;
    S.A[kk][hh][row] = X[((a0 + row) * 2 + hh) * Wm + k0 + kk];
    S.B[kk][hh][row] = X[((b0 + row) * 2 + hh) * Wm + k0 + kk];
  }
}

// the walk over all Wm words: thread (tx, ty) = (tid & 15, tid >> 4) owns rows a0 + ty + 16 r and
// columns b0 + tx + 16 c, and word(ai, bi, aj, bj) takes, word by word, homologues 0 (a) and 1
// (b) of its four rows (i) and four columns (j).  Ends behind a barrier: S may be reused.
template <class Word>
__device__ __forceinline__ void geno_tile64(GenoStage& S, const u64* __restrict__ X, int Wm,
                                            int64_t a0, int64_t b0, Word&& word) {
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  for (int k0 = 0; k0 < Wm; k0 += GRAM_GK) {
    geno_stage_load(S, X, Wm, a0, b0, k0);
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < GRAM_GK; ++kk) {
      u64 ai[4], bi[4], aj[4], bj[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ai[r] = S.A[kk][0][ty + 16 * r];
        bi[r] = S.A[kk][1][ty + 16 * r];
        aj[r] = S.B[kk][0][tx + 16 * r];
        bj[r] = S.B[kk][1][tx + 16 * r];
      }
      word(ai, bi, aj, bj);
    }
    __syncthreads();
  }
}

// acc[r][c] += the dosage dot product of row r and column c over one word
__device__ __forceinline__ void geno_dot16(int (&acc)[4][4], const u64 (&ai)[4],
                                           const u64 (&bi)[4], const u64 (&aj)[4],
                                           const u64 (&bj)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      acc[r][c] += __popcll(ai[r] & aj[c]) + __popcll(ai[r] & bj[c]) +
                   __popcll(bi[r] & aj[c]) + __popcll(bi[r] & bj[c]);
}

// gnx_geno.hip
__global__ void k_geno_rows(int64_t n, const int64_t* __restrict__ slots,
                            const int32_t* __restrict__ grow, int32_t* __restrict__ rows);
// X[i][hom][q] = word widx[q] of row i's homologue, masked (q >= nw and i >= n: 0)
__global__ void k_geno_gather(int64_t n, int64_t n_pad, int nw, int Wm,
                              const int32_t* __restrict__ rows, const int32_t* __restrict__ widx,
                              const u64* __restrict__ wmask, const u64* __restrict__ G, GnxHalves H,
                              u64* __restrict__ X);
// out[i][j] = sum over words and homologue pairs of popcount(X[i][h][w] & X[j][h'][w]) for
// rows i, j < n of X [n rounded up to 64][2][Wm] (rows past n and words past the data: 0)
__global__ void k_geno_gram(int64_t n, int Wm, const u64* __restrict__ X,
                            int64_t* __restrict__ out);

namespace {

// what every entry point checks first: genomes, no ghosts (tiles), the deferred crossover
// joined (the newest offspring's genomes are written) and the living in slots [0, N)
int geno_ready(gnx_state* h, const char* who) {
  if (h->cfg.L == 0 || !h->genomes_assigned) {
    gnx_set_error("%s: genomes not assigned", who);
    return 1;
  }
  if (h->n_ghost > 0) {
    gnx_set_error("%s: the handle holds ghost records (a tile): not supported", who);
    return 1;
  }
  GNXCHK(gnx_xo_join(h));
  GNXCHK(gnx_l_make_dense(h));
  return 0;
}

// the slots' physical genome rows on the device; slots == null: all living slots (n == N).
// d_slots_out (optional): the slots themselves on the device (null when slots == null)
int geno_rows(gnx_state* h, const char* who, int64_t n, const int64_t* slots, GnxScratch& s,
              int32_t** d_rows, int64_t** d_slots_out = nullptr) {
  if (!slots && n != h->N) {
    gnx_set_error("%s: n = %lld but %lld individuals are alive (slots == null)", who,
                  (long long)n, (long long)h->N);
    return 1;
  }
  for (int64_t i = 0; slots && i < n; ++i)
    if (slots[i] < 0 || slots[i] >= h->N) {
      gnx_set_error("%s: slot out of range", who);
      return 1;
    }
  int64_t* d_slots = nullptr;
  GNXCHK(s.get(d_rows, (size_t)n));
  if (slots && n > 0) {
    GNXCHK(s.get(&d_slots, (size_t)n));
    GNXCHK(gnx_h2d(h, d_slots, slots, (size_t)n * sizeof(int64_t)));
  }
  if (n > 0)
    hipLaunchKernelGGL(k_geno_rows, dim3(gnx_grid(n, 256)), dim3(256), 0, h->stream, n, d_slots,
                       h->soa[h->cur].grow, *d_rows);
  HIPCHK(hipGetLastError());
  if (d_slots_out) *d_slots_out = d_slots;
  return 0;
}

// the words that hold a locus of the mask (null: every locus), each with the mask of its loci;
// the padding bits past L never count
void geno_words(gnx_state* h, const uint64_t* locus_mask, std::vector<int32_t>& widx,
                std::vector<u64>& wmask) {
  const int L = h->cfg.L;
  for (int w = 0; w < h->W64; ++w) {
    u64 m = locus_mask ? locus_mask[w] : ~0ull;
    const int64_t lo = (int64_t)w * 64;
    if (lo >= L) m = 0;
    else if (L - lo < 64) m &= (1ull << (L - lo)) - 1ull;
    if (m) {
      widx.push_back(w);
      wmask.push_back(m);
    }
  }
}

// the operand of the 64 x 64 tile kernels on the device
struct GenoOperand {
  u64* X = nullptr;          // [n_pad][2][Wm], written by geno_gather
  int32_t* widx = nullptr;   // [nw]: the genome word behind word q of X
  u64* wmask = nullptr;      // [nw]: the loci of that word that count
  int64_t n_pad = 0;
  int Wm = 0, nw = 0;
};

// the operand's buffers for n_pad rows under the word list, the list uploaded: Wm is the
// multiple of GRAM_GK that leaves at least zero_words words past the nw of the list
int geno_operand(gnx_state* h, GnxScratch& s, int64_t n_pad, const std::vector<int32_t>& widx,
                 const std::vector<u64>& wmask, int zero_words, GenoOperand* op) {
  op->nw = (int)widx.size();
  op->Wm = std::max(GRAM_GK, (op->nw + zero_words + GRAM_GK - 1) / GRAM_GK * GRAM_GK);
  op->n_pad = n_pad;
  GNXCHK(s.get(&op->widx, (size_t)op->nw));
  GNXCHK(s.get(&op->wmask, (size_t)op->nw));
  GNXCHK(s.get(&op->X, (size_t)n_pad * 2 * op->Wm));
  if (op->nw) {
    GNXCHK(gnx_h2d(h, op->widx, widx.data(), op->nw * sizeof(int32_t)));
    GNXCHK(gnx_h2d(h, op->wmask, wmask.data(), op->nw * sizeof(u64)));
  }
  return 0;
}

// the words' three-value tables of gnx_grm and gnx_assoc_quad, [nw_pad][64][4] (nw_pad >= op.nw):
// entry [bit][d] = val[locus][d] for d = 0, 1, 2; zero for the loci outside the mask, the
// padding bits, the words past op.nw and at [bit][3]
std::vector<float> geno_tables(const GenoOperand& op, const std::vector<int32_t>& widx,
                               const std::vector<u64>& wmask, const float* val, int nw_pad) {
  std::vector<float> tab((size_t)nw_pad * 256, 0.f);
  for (int q = 0; q < op.nw; ++q)
    for (int bit = 0; bit < 64; ++bit)
      if ((wmask[q] >> bit) & 1ull) {
        const float* v = val + ((int64_t)widx[q] * 64 + bit) * 3;
        float* t = &tab[((size_t)q * 64 + bit) * 4];
        t[0] = v[0];
        t[1] = v[1];
        t[2] = v[2];
      }
  return tab;
}

// X of the genome rows d_rows [n]: rows n .. n_pad - 1 and words nw .. Wm - 1 are zero
void geno_gather(gnx_state* h, const int32_t* d_rows, int64_t n, const GenoOperand& op) {
  hipLaunchKernelGGL(k_geno_gather, dim3(gnx_grid(op.n_pad * 2 * op.Wm, 256, 256 * 64)),
                     dim3(256), 0, h->stream, n, op.n_pad, op.nw, op.Wm, d_rows, op.widx,
                     op.wmask, (const u64*)h->G, gnx_halves(h), op.X);
}

// G = D D^T of the rows under the mask, exact, into scratch: *d_G int64 [n][n]
int geno_gram_dev(gnx_state* h, GnxScratch& s, const int32_t* d_rows, int64_t n,
                  const uint64_t* locus_mask, int64_t** d_G) {
  std::vector<int32_t> widx;
  std::vector<u64> wmask;
  geno_words(h, locus_mask, widx, wmask);
  const int64_t n_pad = (n + 63) / 64 * 64;
  GenoOperand op;
  GNXCHK(geno_operand(h, s, n_pad, widx, wmask, 0, &op));
  GNXCHK(s.get(d_G, (size_t)n * n));
  geno_gather(h, d_rows, n, op);
  const int T = (int)(n_pad / 64);
  hipLaunchKernelGGL(k_geno_gram, dim3(T, T), dim3(256), 0, h->stream, n, op.Wm, op.X, *d_G);
  return 0;
}

}  // namespace
