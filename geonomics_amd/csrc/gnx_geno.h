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

// words per LDS stage of k_geno_gram: the word count of its operand is a multiple of it
#define GRAM_GK 16

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
