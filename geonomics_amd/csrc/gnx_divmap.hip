// Moving-window diversity sums over a map grid (gnx_divmap_sums, include/gnx_hip.h): per window
// of map cells the four exact integers that pi, heterozygosity, Watterson's theta and Tajima's D
// are host arithmetic on (geonomics_amd/sim/divmap.py) - n, S, sum_het, sum_cc.  Only O(map)
// bytes come back; the per-cell count tables never leave the device.
//
// The genome goes through in locus tiles of whole 64-locus words, a tile so wide that one
// [cell][tile loci] table holds at most max_counts int32.  Per tile three stages:
//   A  k_divmap_counts  the bit-sliced counter of gnx_gc.h (lane = word, chunks of one map
//      cell's individuals) into cnt1 / cnt_het [cell][TL]
//   B  k_divmap_hbox    box sum of half-width r over ix with a running sum along the row,
//      lane = 4 adjacent loci (one 16-byte access), into a second pair of tables
//   C  k_divmap_vstat   box sum over iy with a running sum down a map column, fused with the
//      statistics: a workgroup owns column ix and DM_TPB * 4 loci, forms h, c (2n - c) in 64 bits
//      and the segregating flag at each window, reduces over the wave, adds across waves in LDS
//      and flushes the column's partial sums with integer atomics into [ix][iy] outputs
// Integer adds throughout: the result is exact and independent of the schedule and of the tile
// size.  Loci past L and loci outside the mask are zero in every table (the counter clears
// them, its flush skips l >= L), so c = 0 there: no h, no product, not segregating.
#include "gnx_gc.h"

#define DM_TPB 256                    // threads of stages B and C: 4 waves, 1024 loci
#define DM_NYB 1024                   // windows of a column whose partial sums LDS holds at a time
#define DM_MAX_CELLS (1ll << 20)      // map cells per call
#define DM_MAX_COUNTS (1ll << 26)     // default int32 entries per table (256 MiB), as §14's

// stage A: k_group_counts over the words [tw0, tw0 + tw) of the homologue, the counters of
// loci outside the mask cleared, into tables whose rows are the tile's tw * 64 loci.
// grid (chunks, ceil(tw / GC_TPB))
__global__ void __launch_bounds__(GC_TPB)
k_divmap_counts(int tw0, int tw, int L, const u64* __restrict__ G,
                const int32_t* __restrict__ grow, GnxHalves H, const int32_t* __restrict__ slots,
                const GcChunk* __restrict__ chunks, const u64* __restrict__ mask,
                int32_t* __restrict__ cnt1, int32_t* __restrict__ cnt_het) {
  __shared__ int32_t rows[GC_CHUNK + 1];
  __shared__ u64 pl[(GC_K + 1) * GC_TPB];
  const GcChunk ck = chunks[blockIdx.x];
  gc_load_rows(ck, grow, slots, rows);
  // a lane past the tile's last word reads that word's (its planes are never flushed)
  const int wc = tw0 + min((int)(blockIdx.y * GC_TPB + threadIdx.x), tw - 1);
  u64 px[GC_K], py[GC_K];
  gc_count(ck, rows, G, H, wc, px, py);
  if (mask) {                     // a locus outside the mask: its vertical counters are cleared
    const u64 m = mask[wc];
#pragma unroll
    for (int k = 0; k < GC_K; ++k) {
      px[k] &= m;
      py[k] &= m;
    }
  }
  const int64_t row = (int64_t)ck.g * tw * 64;
  gc_store(pl, px, py, blockIdx.y * GC_TPB + (threadIdx.x >> 6) * 64, tw, L - tw0 * 64,
           cnt1 + row, cnt_het + row);
}

__device__ __forceinline__ int4 dm_add(int4 a, int4 b) {
  return make_int4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ int4 dm_sub(int4 a, int4 b) {
  return make_int4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
}

// stage B: out[iy][ix] = sum of in[iy][ix'] over |ix' - ix| <= r, both tables.  TL4 = the
// tile's loci / 4; a thread owns row iy and 4 loci and walks ix.  grid ny * ceil(TL4 / DM_TPB)
__global__ void __launch_bounds__(DM_TPB)
k_divmap_hbox(int nx, int r, int TL4, int nbx, const int4* __restrict__ in1,
              const int4* __restrict__ inh, int4* __restrict__ out1, int4* __restrict__ outh) {
  const int iy = blockIdx.x / nbx;
  const int q = (blockIdx.x - iy * nbx) * DM_TPB + threadIdx.x;
  if (q >= TL4) return;
  const int64_t base = (int64_t)iy * nx * TL4 + q;
  int4 s1 = make_int4(0, 0, 0, 0), sh = s1;
  for (int ix = 0; ix <= min(r, nx - 1); ++ix) {
    s1 = dm_add(s1, in1[base + (int64_t)ix * TL4]);
    sh = dm_add(sh, inh[base + (int64_t)ix * TL4]);
  }
  for (int ix = 0; ix < nx; ++ix) {
    if (ix > 0) {
      if (ix + r < nx) {                                    // the entering cell
        s1 = dm_add(s1, in1[base + (int64_t)(ix + r) * TL4]);
        sh = dm_add(sh, inh[base + (int64_t)(ix + r) * TL4]);
      }
      if (ix - r - 1 >= 0) {                                // the leaving one
        s1 = dm_sub(s1, in1[base + (int64_t)(ix - r - 1) * TL4]);
        sh = dm_sub(sh, inh[base + (int64_t)(ix - r - 1) * TL4]);
      }
    }
    out1[base + (int64_t)ix * TL4] = s1;
    outh[base + (int64_t)ix * TL4] = sh;
  }
}

template <class T>
__device__ __forceinline__ T dm_wave_sum(T v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// stage C: the windows (iy, ix) of map column ix over this workgroup's 4 DM_TPB loci.  h1 / hh:
// stage B's tables; nwin [ny][nx]: individuals per window; outputs [ix][iy], zeroed before the
// first tile.  grid nx * ceil(TL4 / DM_TPB)
__global__ void __launch_bounds__(DM_TPB)
k_divmap_vstat(int nx, int ny, int r, int TL4, int nbx, const int4* __restrict__ h1,
               const int4* __restrict__ hh, const int32_t* __restrict__ nwin,
               int32_t* __restrict__ out_S, u64* __restrict__ out_het, u64* __restrict__ out_cc) {
  __shared__ u64 a_het[DM_NYB], a_cc[DM_NYB];
  __shared__ int32_t a_S[DM_NYB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int ix = blockIdx.x / nbx;
  const int q = (blockIdx.x - ix * nbx) * DM_TPB + tid;
  const bool live = q < TL4;                 // (a dead lane adds zeros to the wave's sums)
  const int64_t base = (int64_t)ix * TL4 + (live ? q : 0);
  const int64_t pitch = (int64_t)nx * TL4;   // from row iy to row iy + 1
  const int4 zero = make_int4(0, 0, 0, 0);
  int4 s1 = zero, sh = zero;
  if (live)
    for (int iy = 0; iy <= min(r, ny - 1); ++iy) {
      s1 = dm_add(s1, h1[base + iy * pitch]);
      sh = dm_add(sh, hh[base + iy * pitch]);
    }
  for (int y0 = 0; y0 < ny; y0 += DM_NYB) {
    const int yn = min(DM_NYB, ny - y0);
    for (int i = tid; i < yn; i += DM_TPB) {
      a_het[i] = a_cc[i] = 0;
      a_S[i] = 0;
    }
    __syncthreads();
    for (int iy = y0; iy < y0 + yn; ++iy) {
      if (live && iy > 0) {
        if (iy + r < ny) {
          s1 = dm_add(s1, h1[base + (iy + r) * pitch]);
          sh = dm_add(sh, hh[base + (iy + r) * pitch]);
        }
        if (iy - r - 1 >= 0) {
          s1 = dm_sub(s1, h1[base + (iy - r - 1) * pitch]);
          sh = dm_sub(sh, hh[base + (iy - r - 1) * pitch]);
        }
      }
      const int m = 2 * nwin[(int64_t)iy * nx + ix];        // workgroup-uniform
      if (m == 0) continue;                                 // an empty window: every count is 0
      u64 het = (u64)(uint32_t)sh.x + (uint32_t)sh.y + (uint32_t)sh.z + (uint32_t)sh.w;
      u64 cc = (u64)s1.x * (u64)(m - s1.x) + (u64)s1.y * (u64)(m - s1.y) +
               (u64)s1.z * (u64)(m - s1.z) + (u64)s1.w * (u64)(m - s1.w);
      int seg = (s1.x > 0 && s1.x < m) + (s1.y > 0 && s1.y < m) + (s1.z > 0 && s1.z < m) +
                (s1.w > 0 && s1.w < m);
      het = dm_wave_sum(het);
      cc = dm_wave_sum(cc);
      seg = dm_wave_sum(seg);
      if (lane == 0 && (het | cc) != 0) {                   // (seg > 0 implies cc > 0)
        atomicAdd(&a_het[iy - y0], het);
        atomicAdd(&a_cc[iy - y0], cc);
        atomicAdd(&a_S[iy - y0], seg);
      }
    }
    __syncthreads();
    // adjacent lanes, adjacent windows of the column: contiguous in the [ix][iy] outputs
    for (int i = tid; i < yn; i += DM_TPB) {
      const int64_t o = (int64_t)ix * ny + y0 + i;
      if (a_het[i]) atomicAdd(&out_het[o], a_het[i]);
      if (a_cc[i]) atomicAdd(&out_cc[o], a_cc[i]);
      if (a_S[i]) atomicAdd(&out_S[o], a_S[i]);
    }
    __syncthreads();
  }
}

extern "C" int gnx_divmap_info(gnx_state* h, int64_t* tiles, int64_t* chunks, int64_t* launches) {
  if (tiles) *tiles = h->dm_tiles;
  if (chunks) *chunks = h->dm_chunks;
  if (launches) *launches = h->dm_launches;
  return 0;
}

extern "C" int gnx_divmap_sums(gnx_state* h, int64_t n, const int32_t* slots, int32_t nx,
                               int32_t ny, const int64_t* cell_start, int32_t r,
                               const uint64_t* locus_mask, int64_t max_counts, int32_t* out_n,
                               int32_t* out_S, int64_t* out_het, int64_t* out_cc) {
  const char* who = "gnx_divmap_sums";
  if (h->cfg.L == 0 || !h->genomes_assigned) {
    gnx_set_error("%s: genomes not assigned", who);
    return 1;
  }
  if (h->n_ghost > 0) {
    gnx_set_error("%s: the handle holds ghost records (a tile): not supported", who);
    return 1;
  }
  const int L = h->cfg.L, W64 = h->W64, WL = (L + 63) / 64;     // WL: the words that hold loci
  if (nx < 1 || ny < 1) {
    gnx_set_error("%s: nx, ny at least 1 (got %d x %d)", who, (int)nx, (int)ny);
    return 1;
  }
  const int64_t cells = (int64_t)nx * ny;
  if (cells > DM_MAX_CELLS) {
    gnx_set_error("%s: nx * ny = %lld map cells, at most %lld", who, (long long)cells,
                  (long long)DM_MAX_CELLS);
    return 1;
  }
  if (r < 0) {
    gnx_set_error("%s: r >= 0 (got %d)", who, (int)r);
    return 1;
  }
  if (n < 0 || !cell_start || !out_n || !out_S || !out_het || !out_cc || (n > 0 && !slots)) {
    gnx_set_error("%s: null argument or n < 0", who);
    return 1;
  }
  if (cell_start[0] != 0 || cell_start[cells] != n) {
    gnx_set_error("%s: cell_start must start at 0 and end at n = %lld", who, (long long)n);
    return 1;
  }
  for (int64_t c = 0; c < cells; ++c)
    if (cell_start[c + 1] < cell_start[c]) {
      gnx_set_error("%s: cell_start decreases at map cell %lld", who, (long long)c);
      return 1;
    }
  // individuals per window: box sums of the cells' through a summed-area table (rr: r clipped
  // to the map, so that ix + rr cannot overflow)
  std::vector<int64_t> sat((size_t)(nx + 1) * (ny + 1), 0);
  for (int iy = 0; iy < ny; ++iy)
    for (int ix = 0; ix < nx; ++ix) {
      const int64_t c = (int64_t)iy * nx + ix;
      sat[(size_t)(iy + 1) * (nx + 1) + ix + 1] = cell_start[c + 1] - cell_start[c] +
          sat[(size_t)iy * (nx + 1) + ix + 1] + sat[(size_t)(iy + 1) * (nx + 1) + ix] -
          sat[(size_t)iy * (nx + 1) + ix];
    }
  const int rr = std::min<int>(r, std::max(nx, ny));
  std::vector<int32_t> nwin((size_t)cells);
  int64_t n_max = 0;
  for (int iy = 0; iy < ny; ++iy)
    for (int ix = 0; ix < nx; ++ix) {
      const int x0 = std::max(ix - rr, 0), x1 = std::min(ix + rr + 1, (int)nx);
      const int y0 = std::max(iy - rr, 0), y1 = std::min(iy + rr + 1, (int)ny);
      const int64_t v = sat[(size_t)y1 * (nx + 1) + x1] - sat[(size_t)y0 * (nx + 1) + x1] -
                        sat[(size_t)y1 * (nx + 1) + x0] + sat[(size_t)y0 * (nx + 1) + x0];
      if (v >= (1ll << 30)) {
        gnx_set_error("%s: the window of map cell (%d, %d) holds 2^30 individuals or more "
                      "(int32 counts)", who, iy, ix);
        return 1;
      }
      nwin[(size_t)iy * nx + ix] = (int32_t)v;
      n_max = std::max(n_max, v);
    }
  int64_t L_used = L;
  if (locus_mask) {
    L_used = 0;
    for (int w = 0; w < W64; ++w) {
      const int top = L - w * 64;                           // loci of this word below L
      const uint64_t keep = top >= 64 ? ~0ull : top <= 0 ? 0ull : (1ull << top) - 1;
      L_used += __builtin_popcountll(locus_mask[w] & keep);
    }
  }
  if (L_used > 0 && n_max * n_max > INT64_MAX / L_used) {             // (n_max^2 < 2^60)
    gnx_set_error("%s: L' * n_max^2 = %lld * %lld^2 reaches 2^63 (sum_cc is int64)", who,
                  (long long)L_used, (long long)n_max);
    return 1;
  }
  for (int64_t i = 0; i < n; ++i)
    if (slots[i] < 0 || slots[i] >= h->N) {
      gnx_set_error("%s: slot out of range", who);
      return 1;
    }
  GNXCHK(gnx_xo_join(h));
  // the living in slots [0, N).  Defensive, as gnx_stats_group_counts': holes exist only
  // between the steps of a walk, and every exit of a walk gathers the living
  GNXCHK(gnx_l_make_dense(h));
  std::vector<GcChunk> chunks;
  gc_cut_chunks(cells, cell_start, chunks);

  // words per tile: one table holds cells * tw * 64 <= max_counts entries, at least one word
  if (max_counts <= 0) max_counts = DM_MAX_COUNTS;
  const int tw_max = (int)std::max<int64_t>(1, std::min<int64_t>(WL, max_counts / (cells * 64)));
  h->dm_tiles = h->dm_chunks = h->dm_launches = 0;
  for (int64_t c = 0; c < cells; ++c) out_n[c] = nwin[(size_t)c];
  std::fill(out_S, out_S + cells, 0);
  std::fill(out_het, out_het + cells, 0);
  std::fill(out_cc, out_cc + cells, 0);
  if (chunks.empty()) return 0;
  h->dm_chunks = (int64_t)chunks.size();

  GnxScratch sc(who);
  const size_t table = (size_t)cells * tw_max * 64;
  int32_t *c1 = nullptr, *ch = nullptr, *b1 = nullptr, *bh = nullptr, *d_slots = nullptr;
  int32_t *d_nwin = nullptr, *d_S = nullptr;
  u64 *d_het = nullptr, *d_cc = nullptr, *d_mask = nullptr;
  GcChunk* d_chunks = nullptr;
  GNXCHK(sc.get(&c1, table));
  GNXCHK(sc.get(&ch, table));
  GNXCHK(sc.get(&b1, table));
  GNXCHK(sc.get(&bh, table));
  GNXCHK(sc.get(&d_slots, (size_t)n));
  GNXCHK(sc.get(&d_chunks, chunks.size()));
  GNXCHK(sc.get(&d_nwin, (size_t)cells));
  GNXCHK(sc.get(&d_S, (size_t)cells));
  GNXCHK(sc.get(&d_het, (size_t)cells));
  GNXCHK(sc.get(&d_cc, (size_t)cells));
  GNXCHK(gnx_h2d(h, d_slots, slots, (size_t)n * sizeof(int32_t)));
  GNXCHK(gnx_h2d(h, d_chunks, chunks.data(), chunks.size() * sizeof(GcChunk)));
  GNXCHK(gnx_h2d(h, d_nwin, nwin.data(), (size_t)cells * sizeof(int32_t)));
  if (locus_mask) {
    GNXCHK(sc.get(&d_mask, (size_t)W64));
    GNXCHK(gnx_h2d(h, d_mask, locus_mask, (size_t)W64 * sizeof(u64)));
  }
  HIPCHK(hipMemsetAsync(d_S, 0, (size_t)cells * sizeof(int32_t), h->stream));
  HIPCHK(hipMemsetAsync(d_het, 0, (size_t)cells * sizeof(u64), h->stream));
  HIPCHK(hipMemsetAsync(d_cc, 0, (size_t)cells * sizeof(u64), h->stream));
  for (int tw0 = 0; tw0 < WL; tw0 += tw_max) {
    const int tw = std::min(tw_max, WL - tw0);
    const int TL4 = tw * 16, nbx = (TL4 + DM_TPB - 1) / DM_TPB;
    const size_t bytes = (size_t)cells * tw * 64 * sizeof(int32_t);
    HIPCHK(hipMemsetAsync(c1, 0, bytes, h->stream));
    HIPCHK(hipMemsetAsync(ch, 0, bytes, h->stream));
    hipLaunchKernelGGL(k_divmap_counts, dim3((unsigned)chunks.size(), (tw + GC_TPB - 1) / GC_TPB),
                       dim3(GC_TPB), 0, h->stream, tw0, tw, L, (const u64*)h->G,
                       (const int32_t*)h->soa[h->cur].grow, gnx_halves(h),
                       (const int32_t*)d_slots, (const GcChunk*)d_chunks, (const u64*)d_mask, c1,
                       ch);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_divmap_hbox, dim3((unsigned)(ny * nbx)), dim3(DM_TPB), 0, h->stream,
                       (int)nx, rr, TL4, nbx, (const int4*)c1, (const int4*)ch, (int4*)b1,
                       (int4*)bh);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_divmap_vstat, dim3((unsigned)(nx * nbx)), dim3(DM_TPB), 0, h->stream,
                       (int)nx, (int)ny, rr, TL4, nbx, (const int4*)b1, (const int4*)bh,
                       (const int32_t*)d_nwin, d_S, d_het, d_cc);
    HIPCHK(hipGetLastError());
    h->dm_tiles += 1;
    h->dm_launches += 3;
  }
  // [ix][iy] on the device, [iy][ix] for the caller
  std::vector<int32_t> t_S((size_t)cells);
  std::vector<int64_t> t_het((size_t)cells), t_cc((size_t)cells);
  GNXCHK(gnx_d2h(h, t_S.data(), d_S, (size_t)cells * sizeof(int32_t)));
  GNXCHK(gnx_d2h(h, t_het.data(), d_het, (size_t)cells * sizeof(int64_t)));
  GNXCHK(gnx_d2h(h, t_cc.data(), d_cc, (size_t)cells * sizeof(int64_t)));
  for (int iy = 0; iy < ny; ++iy)
    for (int ix = 0; ix < nx; ++ix) {
      const size_t o = (size_t)iy * nx + ix, t = (size_t)ix * ny + iy;
      out_S[o] = t_S[t];
      out_het[o] = t_het[t];
      out_cc[o] = t_cc[t];
    }
  return 0;
}
