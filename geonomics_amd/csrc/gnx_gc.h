// The bit-sliced locus counter shared by gnx_group_counts.hip (per-group tables) and
// gnx_divmap.hip (per-map-cell tables of a locus tile): device functions only.
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
#pragma once
#include <algorithm>
#include <vector>
#include "gnx_internal.h"

typedef unsigned long long u64;

#define GC_K 9                           // planes of a stack
#define GC_CHUNK ((1 << GC_K) - 1)       // individuals per flush (511)
#define GC_U 7                           // individuals in flight = what 3 planes count
#define GC_TPB 256                       // words per workgroup: 4 waves, 4 tiles of 64 words

struct GcChunk {
  int64_t begin;    // first index into slots
  int32_t n;        // 1 .. GC_CHUNK
  int32_t g;        // the group (the map cell) whose table takes the counts
};

// the chunks of groups cut at start[0 .. G]: runs of at most GC_CHUNK individuals of one group
static inline void gc_cut_chunks(int64_t G, const int64_t* start, std::vector<GcChunk>& chunks) {
  for (int64_t g = 0; g < G; ++g)
    for (int64_t s = start[g]; s < start[g + 1]; s += GC_CHUNK)
      chunks.push_back({s, (int32_t)std::min<int64_t>(GC_CHUNK, start[g + 1] - s), (int32_t)g});
}

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
// cnt[64 w + b].  pl: [planes][GC_TPB] of this workgroup, as 32-bit halves.  w0, W64 and L
// count from the first word of cnt's row: the whole homologue, or a locus tile of it
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

// the genome rows of the chunk's individuals into LDS (rows: [GC_CHUNK + 1]); ends in a barrier
__device__ __forceinline__ void gc_load_rows(const GcChunk& ck, const int32_t* __restrict__ grow,
                                             const int32_t* __restrict__ slots, int32_t* rows) {
  for (int i = threadIdx.x; i < ck.n; i += GC_TPB) rows[i] = grow[slots[ck.begin + i]];
  __syncthreads();
}

// the chunk's individuals at word wc (< W64) of both homologues counted into the stacks px
// (heterozygotes) and py (1-1 homozygotes).  An individual past the chunk's end is
// the chunk's last, masked: no branch in the loop, so the GC_U block-table entries and then
// the 2 GC_U words are all in flight together
__device__ __forceinline__ void gc_count(const GcChunk& ck, const int32_t* rows,
                                         const u64* __restrict__ G, const GnxHalves& H, int wc,
                                         u64 (&px)[GC_K], u64 (&py)[GC_K]) {
  // this lane's place in a homologue: block b of the table, word off of the block
  const int b = wc / H.BW;
  const int off = wc - b * H.BW;
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
}

// the stacks through LDS (pl: [(GC_K + 1) * GC_TPB]) into the rows c1 (allele counts) and ch
// (heterozygotes) of the chunk's group; w0, W64, L as gc_flush takes them
__device__ __forceinline__ void gc_store(u64* pl, const u64 (&px)[GC_K], const u64 (&py)[GC_K],
                                         int w0, int W64, int L, int32_t* __restrict__ c1,
                                         int32_t* __restrict__ ch) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
