// What the entry points that read the dosage matrix share (gnx_geno.hip: products over the
// individuals; gnx_gea.hip: cross-products over the loci;
// gnx_mantel.hip: distance cross-sums under permutation): the call's device scratch, the
// preconditions, the slots' genome rows, and the 64 x 64 popcount tile kernel.
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

// device scratch of one call, freed on every exit
struct Scratch {
  std::vector<void*> p;
  ~Scratch() {
    for (void* q : p) (void)hipFree(q);
  }
  template <class T>
  int get(T** out, size_t count) {
    *out = nullptr;
    if (hipMalloc((void**)out, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) {
      gnx_set_error("gnx_geno: out of device memory (%zu bytes)", count * sizeof(T));
      return 1;
    }
    p.push_back(*out);
    return 0;
  }
};

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
int geno_rows(gnx_state* h, const char* who, int64_t n, const int64_t* slots, Scratch& s,
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

}  // namespace
