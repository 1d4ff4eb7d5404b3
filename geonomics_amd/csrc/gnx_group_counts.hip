// Per-group, per-locus counts of 1-alleles and of heterozygotes (gnx_stats_group_counts,
// include/gnx_hip.h): what Fst between groups of individuals, per-group diversity and the
// site-frequency spectrum are host arithmetic on (geonomics_amd/sim/fst.py).  It replaces the
// reference's route - download every genotype, then loop in Python over loci x pairs of
// islands (tests/validation/island/island_test.py:70-115).
//
// The counter itself - lane = one 64-locus word, bit-sliced planes, chunks of at most GC_CHUNK
// individuals of one group flushed through LDS into integer atomics - is gnx_gc.h's.
#include "gnx_gc.h"

#define GC_MAX_GROUPS 1024
#define GC_MAX_CELLS (1ll << 26)         // G * L counts per table (256 MiB each)

__global__ void __launch_bounds__(GC_TPB)
k_group_counts(int W64, int L, const u64* __restrict__ G, const int32_t* __restrict__ grow,
               GnxHalves H, const int32_t* __restrict__ slots,
               const GcChunk* __restrict__ chunks, int32_t* __restrict__ cnt1,
               int32_t* __restrict__ cnt_het) {
  __shared__ int32_t rows[GC_CHUNK + 1];
  __shared__ u64 pl[(GC_K + 1) * GC_TPB];
  const GcChunk ck = chunks[blockIdx.x];
  gc_load_rows(ck, grow, slots, rows);
  // a lane past the last word reads the last word's (its planes are never flushed)
  const int w = blockIdx.y * GC_TPB + threadIdx.x;
  u64 px[GC_K], py[GC_K];
  gc_count(ck, rows, G, H, min(w, W64 - 1), px, py);
  gc_store(pl, px, py, blockIdx.y * GC_TPB + (threadIdx.x >> 6) * 64, W64, L,
           cnt1 + (int64_t)ck.g * L, cnt_het + (int64_t)ck.g * L);
}

extern "C" int gnx_stats_group_counts(gnx_state* h, int64_t n, const int32_t* slots, int32_t G,
                                      const int64_t* group_start, int32_t* cnt1,
                                      int32_t* cnt_het) {
  const char* who = "gnx_stats_group_counts";
  if (h->cfg.L == 0 || !h->genomes_assigned) {
    gnx_set_error("%s: genomes not assigned", who);
    return 1;
  }
  if (h->n_ghost > 0) {
    gnx_set_error("%s: the handle holds ghost records (a tile): not supported", who);
    return 1;
  }
  const int L = h->cfg.L;
  if (G < 1 || G > GC_MAX_GROUPS) {
    gnx_set_error("%s: 1..%d groups per call (got %d)", who, GC_MAX_GROUPS, (int)G);
    return 1;
  }
  if ((int64_t)G * L > GC_MAX_CELLS) {
    gnx_set_error("%s: G * L = %lld counts per table, at most %lld", who, (long long)G * L,
                  (long long)GC_MAX_CELLS);
    return 1;
  }
  if (n < 0 || !group_start || !cnt1 || !cnt_het || (n > 0 && !slots)) {
    gnx_set_error("%s: null argument or n < 0", who);
    return 1;
  }
  if (group_start[0] != 0 || group_start[G] != n) {
    gnx_set_error("%s: group_start must start at 0 and end at n = %lld", who, (long long)n);
    return 1;
  }
  for (int g = 0; g < G; ++g) {
    if (group_start[g + 1] < group_start[g]) {
      gnx_set_error("%s: group_start decreases at group %d", who, g);
      return 1;
    }
    if (group_start[g + 1] - group_start[g] >= (1ll << 30)) {
      gnx_set_error("%s: group %d holds 2^30 individuals or more (int32 counts)", who, g);
      return 1;
    }
  }
  for (int64_t i = 0; i < n; ++i)
    if (slots[i] < 0 || slots[i] >= h->N) {
      gnx_set_error("%s: slot out of range", who);
      return 1;
    }
  GNXCHK(gnx_xo_join(h));
  // the living in slots [0, N).  Defensive, as geno_ready's: holes exist only between the steps
  // of a walk, and every exit of a walk, the failing one included, gathers the living
  GNXCHK(gnx_l_make_dense(h));
  std::vector<GcChunk> chunks;
  gc_cut_chunks(G, group_start, chunks);

  GnxScratch sc(who);
  const size_t cells = (size_t)G * L;
  int32_t *d1 = nullptr, *d2 = nullptr, *d_slots = nullptr;
  GcChunk* d_chunks = nullptr;
  GNXCHK(sc.get(&d1, cells));
  GNXCHK(sc.get(&d2, cells));
  HIPCHK(hipMemsetAsync(d1, 0, cells * sizeof(int32_t), h->stream));
  HIPCHK(hipMemsetAsync(d2, 0, cells * sizeof(int32_t), h->stream));
  if (!chunks.empty()) {
    GNXCHK(sc.get(&d_slots, (size_t)n));
    GNXCHK(sc.get(&d_chunks, chunks.size()));
    GNXCHK(gnx_h2d(h, d_slots, slots, (size_t)n * sizeof(int32_t)));
    GNXCHK(gnx_h2d(h, d_chunks, chunks.data(), chunks.size() * sizeof(GcChunk)));
    hipLaunchKernelGGL(k_group_counts, dim3((unsigned)chunks.size(), (h->W64 + GC_TPB - 1) / GC_TPB),
                       dim3(GC_TPB), 0, h->stream, h->W64, L, (const u64*)h->G,
                       (const int32_t*)h->soa[h->cur].grow, gnx_halves(h),
                       (const int32_t*)d_slots, (const GcChunk*)d_chunks, d1, d2);
    HIPCHK(hipGetLastError());
  }
  GNXCHK(gnx_d2h(h, cnt1, d1, cells * sizeof(int32_t)));
  GNXCHK(gnx_d2h(h, cnt_het, d2, cells * sizeof(int32_t)));
  return 0;
}
