// Per-group, per-locus counts of 1-alleles and of heterozygotes (gnx_stats_group_counts,
// include/gnx_hip.h): what Fst between groups of individuals, per-group diversity and the
// site-frequency spectrum are host arithmetic on (geonomics_amd/sim/fst.py).  It replaces the
// reference's route - download every genotype, then loop in Python over loci x pairs of
// islands (tests/validation/island/island_test.py:70-115).
//
// Lane = one 64-locus word of a homologue, so a wave reads 512 contiguous bytes per homologue
// (apart from block boundaries: the block-table entry is per lane).  A lane counts its 64 loci
// bit-sliced: a stack of 64-bit planes is 64 vertical counters, plane k holding bit k of each.
// Two stacks: x = a ^ b (heterozygotes) and y = a & b (1-1 homozygotes); the allele count is
// x + 2 y, formed once per flush by a bit-sliced add.  GC_U individuals' words are loaded
// before the first add and go into a 3-plane stack first (GC_U = 7 = 2^3 - 1), which is then
// added to the GC_K-plane stack: a full ripple per individual would make the kernel
// ALU-bound.  A chunk is a run of at most GC_CHUNK = 2^GC_K - 1 individuals of one group, cut
// on the host; after it the planes go through LDS, where lane b of a wave picks bit b of each
// word of the wave in turn: one int32 atomicAdd per lane into 64 adjacent counts, 256
// contiguous bytes per wave instruction, at most 16 of them outstanding per wave.  Integer
// adds: exact, whatever the schedule.
#include <algorithm>
#include <vector>
#include "gnx_internal.h"

typedef unsigned long long u64;

#define GC_K 9                           // planes of a stack
#define GC_CHUNK ((1 << GC_K) - 1)       // individuals per flush (511)
#define GC_U 7                           // individuals in flight = what 3 planes count
#define GC_TPB 256                       // words per workgroup: 4 waves, 4 tiles of 64 words
#define GC_MAX_GROUPS 1024
#define GC_MAX_CELLS (1ll << 26)         // G * L counts per table (256 MiB each)

struct GcChunk {
  int64_t begin;    // first index into slots
  int32_t n;        // 1 .. GC_CHUNK
  int32_t g;
};

// planes += the 3-plane number s (s0 weight 1): full adders, then the carry ripples on
__device__ __forceinline__ void gc_add3(u64 (&p)[GC_K], u64 s0, u64 s1, u64 s2) {
  u64 c = p[0] & s0;
  p[0] ^= s0;
  u64 t = p[1] ^ s1;
  u64 c2 = (p[1] & s1) | (t & c);
  p[1] = t ^ c;
  t = p[2] ^ s2;
  c = (p[2] & s2) | (t & c2);
  p[2] = t ^ c2;
#pragma unroll
  for (int k = 3; k < GC_K; ++k) {
    t = p[k] & c;
    p[k] ^= c;
    c = t;
  }
}

// the wave's 64 words, one after the other: lane b adds bit b of the word's planes to
// cnt[64 w + b].  pl: [planes][GC_TPB] of this workgroup, as 32-bit halves
template <int P>
__device__ __forceinline__ void gc_flush(const uint32_t* pl, int wave, int lane, int w0, int W64,
                                         int L, int32_t* __restrict__ cnt) {
  const int half = lane >> 5, sh = lane & 31;
  for (int j = 0; j < 64; ++j) {
    const int w = w0 + j;
    if (w >= W64) break;                                     // wave-uniform
    int c = 0;
#pragma unroll
    for (int k = 0; k < P; ++k)
      c |= (int)((pl[(k * GC_TPB + wave * 64 + j) * 2 + half] >> sh) & 1u) << k;
    const int l = w * 64 + lane;
    if (__ballot(c != 0) != 0ull && l < L) atomicAdd(&cnt[l], c);
    // at most 16 atomics of this wave outstanding: beyond that the issue stalls anyway
    asm volatile("s_waitcnt vmcnt(15)" ::: "memory");
  }
}

__global__ void __launch_bounds__(GC_TPB)
k_group_counts(int W64, int L, const u64* __restrict__ G, const int32_t* __restrict__ grow,
               GnxHalves H, const int32_t* __restrict__ slots,
               const GcChunk* __restrict__ chunks, int32_t* __restrict__ cnt1,
               int32_t* __restrict__ cnt_het) {
  __shared__ int32_t rows[GC_CHUNK + 1];
  __shared__ u64 pl[(GC_K + 1) * GC_TPB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const GcChunk ck = chunks[blockIdx.x];
  const int w = blockIdx.y * GC_TPB + tid;
  for (int i = tid; i < ck.n; i += GC_TPB) rows[i] = grow[slots[ck.begin + i]];
  __syncthreads();

  // this lane's place in a homologue: block b of the table, word off of the block.  A lane
  // past the last word reads the last word's (its planes are never flushed), and an
  // individual past the chunk's end is the chunk's last, masked: no branch in the loop, so
  // the GC_U block-table entries and then the 2 GC_U words are all in flight together
  const int wc = min(w, W64 - 1);
  const int b = wc / H.BW;
  const int off = wc - b * H.BW;
  u64 px[GC_K], py[GC_K];
#pragma unroll
  for (int k = 0; k < GC_K; ++k) px[k] = py[k] = 0;

  for (int i0 = 0; i0 < ck.n; i0 += GC_U) {
    int32_t e0[GC_U], e1[GC_U];
#pragma unroll
    for (int u = 0; u < GC_U; ++u) {
      const int64_t lb = (int64_t)rows[min(i0 + u, ck.n - 1)] * 2 * H.NB + b;
      e0[u] = H.hmap[lb];
      e1[u] = H.hmap[lb + H.NB];
    }
    u64 va[GC_U], vb[GC_U];
#pragma unroll
    for (int u = 0; u < GC_U; ++u) {
      va[u] = G[(int64_t)GNX_BLK(e0[u]) * H.BW + off];
      vb[u] = G[(int64_t)GNX_BLK(e1[u]) * H.BW + off];
    }
#pragma unroll
    for (int u = 0; u < GC_U; ++u) {
      const u64 m = i0 + u < ck.n ? ~0ull : 0ull;
      va[u] &= m;
      vb[u] &= m;
    }
    u64 x0 = 0, x1 = 0, x2 = 0, y0 = 0, y1 = 0, y2 = 0;
#pragma unroll
    for (int u = 0; u < GC_U; ++u) {
      u64 x = va[u] ^ vb[u], y = va[u] & vb[u], t;
      t = x0 & x; x0 ^= x; x = t;
      t = x1 & x; x1 ^= x; x2 ^= t;
      t = y0 & y; y0 ^= y; y = t;
      t = y1 & y; y1 ^= y; y2 ^= t;
    }
    gc_add3(px, x0, x1, x2);
    gc_add3(py, y0, y1, y2);
  }

  int32_t* c1 = cnt1 + (int64_t)ck.g * L;
  int32_t* ch = cnt_het + (int64_t)ck.g * L;
  const int w0 = blockIdx.y * GC_TPB + wave * 64;
#pragma unroll
  for (int k = 0; k < GC_K; ++k) pl[k * GC_TPB + tid] = px[k];
  __syncthreads();
  gc_flush<GC_K>((const uint32_t*)pl, wave, lane, w0, W64, L, ch);
  __syncthreads();
  // the allele count x + 2 y, bit-sliced: plane 0 is x's, plane k adds x_k, y_(k-1) and a carry
  pl[tid] = px[0];
  u64 c = 0;
#pragma unroll
  for (int k = 1; k < GC_K; ++k) {
    const u64 t = px[k] ^ py[k - 1];
    pl[k * GC_TPB + tid] = t ^ c;
    c = (px[k] & py[k - 1]) | (t & c);
  }
  pl[GC_K * GC_TPB + tid] = py[GC_K - 1] ^ c;       // at most 2 GC_CHUNK < 2^(GC_K + 1)
  __syncthreads();
  gc_flush<GC_K + 1>((const uint32_t*)pl, wave, lane, w0, W64, L, c1);
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
  for (int g = 0; g < G; ++g)
    for (int64_t s = group_start[g]; s < group_start[g + 1]; s += GC_CHUNK)
      chunks.push_back({s, (int32_t)std::min<int64_t>(GC_CHUNK, group_start[g + 1] - s), g});

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
