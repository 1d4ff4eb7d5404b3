// Genome-wide linkage disequilibrium on the device: per bin of the distance between two loci the
// number of locus pairs and the sums of r^2, r^4, the distance and (map distances) Weir & Hill's
// drift weight, from which the decay of r^2 with recombination distance and the LD estimate of
// the effective population size follow on the host (geonomics_amd/sim/ld.py).  Both are
// reductions over the locus pairs: nothing n_loci x n_loci exists anywhere, so the call takes any
// number of loci (gnx_stats_ld, the reference's _calc_ld pair by pair, stops at 8192).
//
//   gnx_ld_bins    c1 [n_loci] int64, pairs [n_bins] int64, fsums [n_bins][4] fp64, work
//
// Pass 1, k_ld_bits: T[j][q] = the bits of the sampled chromosomes 64 q .. 64 q + 63 (chromosome
// = 2 * sample index + homologue) at locus loci[j] - the layout of k_ld_transpose (gnx_stats.hip)
// with the rows padded to whole stages.  A wave takes 64 chromosomes and one 128-byte line of
// their homologues at a time: eight 16-byte loads per lane, eight lanes per row, so every wave
// instruction reads eight whole lines (gnx_chunk_at); the line goes through LDS (row pitch 17
// words: no bank conflict either way) so that lane = chromosome holds one genome word, and
// __ballot((v >> b) & 1) is the transposed word of locus 64 w + b.  Words without a requested
// locus are skipped after the load; every genome line of the sample that holds a requested locus
// is read once.  k_ld_rowsum takes c1[j], the popcount of row j.
//
// When the bit rows as allocated (whole tiles x padded words x 8) exceed the byte budget
// (gnx_ld_budget, 256 MiB by default) the loci
// are worked off in blocks of whole 64-locus tiles, two blocks resident at a time: block bi in
// buffer A against itself, then against every later block bj in buffer B that shares a listed
// tile with it.
//
// Pass 2, k_ld_pairs: a task is a tile of 64 x 64 loci (i-tile <= j-tile; on the diagonal only
// i < j).  The host lists only the tiles whose distance range meets [edges[0], edges[last]) -
// the loci are ordered by pos, so a band-limited request costs its band.  A fixed grid of
// workgroups: workgroup g takes tasks g, g + grid, ...  The body is the LDS-staged popcount tile
// of k_geno_gram on single bit rows: stages of LD_K chromosome words of both tiles, thread
// (tx, ty) keeps c_ij of rows ty + 16 r and columns tx + 16 c in int32 registers, so every staged
// word is used 64 times.  The epilogue takes the thread's sixteen pairs one at a time: r^2 from
// integers (see include/gnx_hip.h), the bin of pos[j] - pos[i], then for every bin present in
// the wave the wave adds its lanes' terms of that bin by an xor butterfly and lane 0 adds the
// result to the wave's accumulators in LDS.  A workgroup leaves one partial (its
// four waves in wave order); k_ld_total adds the partials of a launch in workgroup order to the
// running totals.  No floating-point atomics: the order of every fp64 sum is fixed by the
// arguments (and the byte budget), so a call repeated is bit-equal.
#include <cmath>
#include "gnx_geno.h"

#define LD_K 16                   // chromosome words per LDS stage
#define LD_NB 64                  // bins at most
#define LD_NF 4                   // fp64 sums per bin: r^2, r^4, d, w
#define LD_BLOCKS 2048            // workgroups of the pair kernel at most (one partial each)
#define LD_BUDGET (256ll << 20)   // bytes of bit rows resident unless gnx_ld_budget says so
#define LD_MAX_CHROM (1ll << 26)  // n c_ij - c_i c_j stays below 2^52: exact in fp64

struct alignas(16) LdChunk {
  u64 a, b;
};

struct LdTask {
  int32_t ti, tj;                 // tiles of 64 loci (indices into the request), ti <= tj
};

// see the head of the file.  lines[n_lines]: the 128-byte lines (16 genome words) that hold a
// requested locus of this block; jof[W64 * 64]: locus -> index in the request, or -1; the block
// is the request's indices j0 .. j0 + nj - 1, row j - j0 of T (row pitch `pitch` words)
__global__ void __launch_bounds__(256)
k_ld_bits(int64_t n_chrom, int64_t nq, int64_t pitch, int n_lines,
          const int32_t* __restrict__ lines, const int32_t* __restrict__ rows,
          const LdChunk* __restrict__ G, GnxHalves H, int W64, const int32_t* __restrict__ jof,
          int j0, int nj, u64* __restrict__ T) {
  __shared__ u64 tile[4][64][17];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + wave;
  const bool live = q < nq;                           // wave-uniform
  for (int li = blockIdx.y; li < n_lines; li += gridDim.y) {
    const int line = lines[li];
    __syncthreads();                                  // the last line's words have been read
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int r = s * 8 + (lane >> 3), cc = lane & 7;
      const int64_t chrom = q * 64 + r;
      LdChunk v{0ull, 0ull};
      if (live && chrom < n_chrom)
        v = G[gnx_chunk_at(H, (int64_t)rows[chrom >> 1] * 2 + (chrom & 1), line * 8 + cc)];
      tile[wave][r][2 * cc] = v.a;
      tile[wave][r][2 * cc + 1] = v.b;
    }
    __syncthreads();
    if (!live) continue;
    for (int wi = 0; wi < 16; ++wi) {
      const int w = line * 16 + wi;
      if (w >= W64) break;
      const int jj = jof[(int64_t)w * 64 + lane] - j0;
      const bool want = jj >= 0 && jj < nj;
      if (__ballot(want) == 0ull) continue;           // wave-uniform
      const u64 v = tile[wave][lane][wi];
      u64 mine = 0;
#pragma unroll 8
      for (int b = 0; b < 64; ++b) {
        const u64 bal = __ballot((v >> b) & 1ull);
        if (lane == b) mine = bal;
      }
      if (want) T[(int64_t)jj * pitch + q] = mine;
    }
  }
}

// c1[row] = the popcount of row `row` of T (one wave per row)
__global__ void __launch_bounds__(256)
k_ld_rowsum(int nj, int64_t nq, int64_t pitch, const u64* __restrict__ T,
            long long* __restrict__ c1) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nj) return;                              // wave-uniform
  long long s = 0;
  for (int64_t q = lane; q < nq; q += 64) s += __popcll(T[(int64_t)row * pitch + q]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0) c1[row] = s;
}

__device__ __forceinline__ double ld_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ long long ld_wave_sum(long long v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// ipart[g][LD_NB] = pairs per bin, fpart[g][LD_NB][LD_NF] = {sum r^2, sum r^4, sum d, sum w}.
// Tile t of the request is rows (t - tA0) * 64 .. of TA as an i-tile and (t - tB0) * 64 .. of
// TB as a j-tile; n = the sampled chromosomes, mm = max(1, min_minor)
__global__ void __launch_bounds__(256)
k_ld_pairs(int64_t n_tasks, const LdTask* __restrict__ tasks, int64_t pitch, int n_loci,
           const u64* __restrict__ TA, int tA0, const u64* __restrict__ TB, int tB0, long long n,
           long long mm, int morgans, int n_bins, const long long* __restrict__ c1,
           const double* __restrict__ pos, const double* __restrict__ edges,
           long long* __restrict__ ipart, double* __restrict__ fpart) {
  __shared__ u64 As[LD_K][65];
  __shared__ u64 Bs[LD_K][65];
  __shared__ double E[LD_NB + 1];
  __shared__ long long cc[2][64];
  __shared__ double pp[2][64];
  __shared__ long long Iw[4][LD_NB];
  __shared__ double Fw[4][LD_NB][LD_NF];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, wave = tid >> 6, lane = tid & 63;
  for (int q = tid; q < 4 * LD_NB; q += 256) (&Iw[0][0])[q] = 0;
  for (int q = tid; q < 4 * LD_NB * LD_NF; q += 256) (&Fw[0][0][0])[q] = 0.0;
  if (tid <= n_bins) E[tid] = edges[tid];
  for (int64_t t = blockIdx.x; t < n_tasks; t += gridDim.x) {
    const LdTask K = tasks[t];
    __syncthreads();                                  // the last task's epilogue has read cc, pp
    if (tid < 128) {
      const int side = tid >> 6, i = tid & 63;
      const int64_t g = (int64_t)(side ? K.tj : K.ti) * 64 + i;
      cc[side][i] = g < n_loci ? c1[g] : 0;           // past the request: never kept
      pp[side][i] = g < n_loci ? pos[g] : 0.0;
    }
    const u64* a = TA + (int64_t)(K.ti - tA0) * 64 * pitch;
    const u64* b = TB + (int64_t)(K.tj - tB0) * 64 * pitch;
    int acc[4][4] = {};
    for (int64_t k0 = 0; k0 < pitch; k0 += LD_K) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int q = tid + 256 * s;                  // (row, 16-byte chunk) with the chunk fastest
        const int row = q >> 3, c2 = (q & 7) * 2;
        const LdChunk va = *(const LdChunk*)(a + (int64_t)row * pitch + k0 + c2);
        const LdChunk vb = *(const LdChunk*)(b + (int64_t)row * pitch + k0 + c2);
        As[c2][row] = va.a;
        As[c2 + 1][row] = va.b;
        Bs[c2][row] = vb.a;
        Bs[c2 + 1][row] = vb.b;
      }
      __syncthreads();
#pragma unroll 4
      for (int kk = 0; kk < LD_K; ++kk) {
        u64 ai[4], bj[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ai[r] = As[kk][ty + 16 * r];
          bj[r] = Bs[kk][tx + 16 * r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] += __popcll(ai[r] & bj[c]);
      }
      __syncthreads();
    }
    // ---- epilogue, one of the thread's sixteen pairs at a time (all at once take more
    // registers than the main loop)
    const bool diag = K.ti == K.tj;
#pragma unroll 1
    for (int rc = 0; rc < 16; ++rc) {
      const int r = rc >> 2, c = rc & 3;
      const int i = ty + 16 * r, j = tx + 16 * c;
      int cij = 0;
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (q == rc) cij = acc[q >> 2][q & 3];
      const long long ci = cc[0][i], cj = cc[1][j];
      const double d = pp[1][j] - pp[0][i];
      int bin = -1;
      if (min(ci, n - ci) >= mm && min(cj, n - cj) >= mm && (!diag || i < j) && d >= E[0] &&
          d < E[n_bins]) {
        int lo = 0, hi = n_bins;
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (d >= E[mid]) lo = mid;
          else hi = mid;
        }
        bin = lo;
      }
      double r2 = 0.0, ww = 0.0;
      u64 present = 0;
      if (bin >= 0) {
        const double dn = (double)(n * (long long)cij - ci * cj);
        r2 = (dn * dn) / ((double)(ci * (n - ci)) * (double)(cj * (n - cj)));
        if (morgans) {
          // d >= 0: |.| only keeps a library expm1(-0) = +0 from making c = -0, w = -inf
          const double rf = 0.5 * fabs(expm1(-2.0 * d));
          ww = ((1.0 - rf) * (1.0 - rf) + rf * rf) / ((2.0 * rf) * (2.0 - rf));
        }
        present = 1ull << bin;
      }
#pragma unroll
      for (int s = 32; s > 0; s >>= 1)
        present |= (u64)__shfl_xor((long long)present, s, 64);
      unsigned plo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)present);
      unsigned phi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(present >> 32));
      while (plo | phi) {                             // wave-uniform: the bins in the wave
        int k;
        if (plo) {
          k = __ffs((int)plo) - 1;
          plo &= plo - 1;
        } else {
          k = 32 + __ffs((int)phi) - 1;
          phi &= phi - 1;
        }
        const bool in = bin == k;
        const long long ic = ld_wave_sum((long long)(in ? 1 : 0));
        const double f0 = ld_wave_sum(in ? r2 : 0.0);
        const double f1 = ld_wave_sum(in ? r2 * r2 : 0.0);
        const double f2 = ld_wave_sum(in ? d : 0.0);
        const double f3 = ld_wave_sum(in ? ww : 0.0);
        if (lane == 0) {
          Iw[wave][k] += ic;
          Fw[wave][k][0] += f0;
          Fw[wave][k][1] += f1;
          Fw[wave][k][2] += f2;
          Fw[wave][k][3] += f3;
        }
      }
    }
  }
  __syncthreads();
  for (int q = tid; q < LD_NB; q += 256) {
    const long long* p = &Iw[0][0] + q;
    ipart[(int64_t)blockIdx.x * LD_NB + q] = p[0] + p[LD_NB] + p[2 * LD_NB] + p[3 * LD_NB];
  }
  for (int q = tid; q < LD_NB * LD_NF; q += 256) {
    const double* p = &Fw[0][0][0] + q;
    const int m = LD_NB * LD_NF;
    fpart[(int64_t)blockIdx.x * m + q] = ((p[0] + p[m]) + p[2 * m]) + p[3 * m];
  }
}

// the partials of one launch added to the running totals in workgroup order
__global__ void k_ld_total(int blocks, const long long* __restrict__ ipart,
                           const double* __restrict__ fpart, long long* __restrict__ itot,
                           double* __restrict__ ftot) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int mf = LD_NB * LD_NF;
  if (q < LD_NB) {
    long long s = itot[q];
    for (int g = 0; g < blocks; ++g) s += ipart[(int64_t)g * LD_NB + q];
    itot[q] = s;
  } else if (q < LD_NB + mf) {
    const int c = q - LD_NB;
    double s = ftot[c];
    for (int g = 0; g < blocks; ++g) s += fpart[(int64_t)g * mf + c];
    ftot[c] = s;
  }
}

// buf [buf_words], zeroed here, = the bit rows of the request's indices ja .. ja + nj - 1 (row
// pitch `pitch` words; rows past nj and words past the sample stay 0); lines[n_lines]: the genome
// lines that hold one of them; c1 != null: c1[0 .. nj) = their popcounts.  -> kernels launched
int ld_transpose(gnx_state* h, int64_t n_chrom, int64_t nq, int64_t pitch, int n_lines,
                 const int32_t* d_lines, const int32_t* d_rows, const int32_t* d_jof, int ja,
                 int nj, u64* buf, int64_t buf_words, long long* c1) {
  (void)hipMemsetAsync(buf, 0, (size_t)buf_words * sizeof(u64), h->stream);
  hipLaunchKernelGGL(k_ld_bits, dim3((unsigned)((nq + 3) / 4), (unsigned)std::min(n_lines, 64)),
                     dim3(256), 0, h->stream, n_chrom, nq, pitch, n_lines, d_lines, d_rows,
                     (const LdChunk*)h->G, gnx_halves(h), h->W64, d_jof, ja, nj, buf);
  if (!c1) return 1;
  hipLaunchKernelGGL(k_ld_rowsum, dim3((unsigned)((nj + 3) / 4)), dim3(256), 0, h->stream, nj, nq,
                     pitch, buf, c1);
  return 2;
}

// see gnx_internal.h: the bit rows of a whole request at once, for the callers outside this file
int gnx_ld_bit_rows(gnx_state* h, GnxScratch& s, GnxCallTimer& tm, const int32_t* d_rows,
                    int64_t n_chrom, int32_t n_loci, const int32_t* loci,
                    const std::vector<int32_t>& jof, unsigned long long** T, int64_t* pitch_out,
                    long long** c1) {
  const int64_t nq = (n_chrom + 63) / 64;
  const int64_t pitch = (nq + LD_K - 1) / LD_K * LD_K;
  std::vector<int32_t> lines((size_t)n_loci);
  for (int j = 0; j < n_loci; ++j) lines[(size_t)j] = loci[j] >> 10;
  std::sort(lines.begin(), lines.end());
  lines.erase(std::unique(lines.begin(), lines.end()), lines.end());
  int32_t *d_jof = nullptr, *d_lines = nullptr;
  GNXCHK(s.get(T, (size_t)n_loci * pitch));
  GNXCHK(s.get(c1, (size_t)n_loci));
  GNXCHK(s.get(&d_jof, jof.size()));
  GNXCHK(s.get(&d_lines, lines.size()));
  GNXCHK(gnx_h2d(h, d_jof, jof.data(), jof.size() * sizeof(int32_t)));
  GNXCHK(gnx_h2d(h, d_lines, lines.data(), lines.size() * sizeof(int32_t)));
  tm.start();
  const int launches = ld_transpose(h, n_chrom, nq, pitch, (int)lines.size(), d_lines, d_rows,
                                    d_jof, 0, n_loci, *T, (int64_t)n_loci * pitch, *c1);
  HIPCHK(hipGetLastError());
  GNXCHK(tm.stop(launches));
  *pitch_out = pitch;
  return 0;
}

extern "C" int gnx_ld_budget(gnx_state* h, int64_t bytes) {
  if (bytes < 0) {
    gnx_set_error("gnx_ld_budget: bytes >= 0 (0: the default)");
    return 1;
  }
  h->ld_budget = bytes;
  return 0;
}

extern "C" int gnx_ld_info(gnx_state* h, double* kernel_ms, int64_t* launches,
                           int64_t* locus_blocks) {
  if (kernel_ms) *kernel_ms = h->ld_ms;
  if (launches) *launches = h->ld_launches;
  if (locus_blocks) *locus_blocks = h->ld_blocks;
  return 0;
}

extern "C" int gnx_ld_bins(gnx_state* h, int64_t n, const int64_t* slots, int32_t n_loci,
                           const int32_t* loci, const double* pos, int32_t n_edges,
                           const double* edges, int32_t min_minor, int32_t morgans,
                           int64_t max_work, int64_t* work, int64_t* c1, int64_t* pairs,
                           double* fsums) {
  const char* who = "gnx_ld_bins";
  h->ld_ms = 0.0;
  h->ld_launches = 0;
  h->ld_blocks = 0;
  GNXCHK(geno_ready(h, who));
  if (n < 1 || 2 * n > LD_MAX_CHROM) {
    gnx_set_error("%s: 1..2^25 individuals (2^26 chromosomes) per call (got %lld)", who,
                  (long long)n);
    return 1;
  }
  if (!slots && n != h->N) {
    gnx_set_error("%s: n = %lld but %lld individuals are alive (slots == null)", who,
                  (long long)n, (long long)h->N);
    return 1;
  }
  if (slots) {
    std::vector<bool> seen((size_t)h->N, false);
    for (int64_t i = 0; i < n; ++i) {
      if (slots[i] < 0 || slots[i] >= h->N) {
        gnx_set_error("%s: slot out of range", who);
        return 1;
      }
      if (seen[(size_t)slots[i]]) {
        gnx_set_error("%s: slot %lld is listed twice", who, (long long)slots[i]);
        return 1;
      }
      seen[(size_t)slots[i]] = true;
    }
  }
  const int L = h->cfg.L, W64 = h->W64;
  if (n_loci < 1 || !loci || !pos) {
    gnx_set_error("%s: at least one locus, with its position (n_loci = %d)", who, n_loci);
    return 1;
  }
  if (n_edges < 2 || n_edges > LD_NB + 1 || !edges) {
    gnx_set_error("%s: 2..%d edges (got %d)", who, LD_NB + 1, n_edges);
    return 1;
  }
  if (!work || (max_work > 0 && (!c1 || !pairs || !fsums))) {
    gnx_set_error("%s: null work or output", who);
    return 1;
  }
  const int n_bins = n_edges - 1;
  for (int k = 0; k < n_edges; ++k) {
    const bool last = k == n_edges - 1;
    if (std::isnan(edges[k]) || (!last && !std::isfinite(edges[k])) || edges[k] == -INFINITY ||
        (k > 0 && !(edges[k] > edges[k - 1]))) {
      gnx_set_error("%s: edges must be ascending and finite (the last may be +inf) "
                    "(edges[%d] = %g)", who, k, edges[k]);
      return 1;
    }
  }
  std::vector<int32_t> jof((size_t)W64 * 64, -1);
  for (int j = 0; j < n_loci; ++j) {
    if (loci[j] < 0 || loci[j] >= L) {
      gnx_set_error("%s: locus out of range (loci[%d] = %d)", who, j, loci[j]);
      return 1;
    }
    if (jof[(size_t)loci[j]] >= 0) {
      gnx_set_error("%s: locus %d is listed twice", who, loci[j]);
      return 1;
    }
    jof[(size_t)loci[j]] = j;
    if (!std::isfinite(pos[j]) || (j > 0 && !(pos[j] >= pos[j - 1]))) {
      gnx_set_error("%s: pos must be finite and non-decreasing (pos[%d] = %g)", who, j, pos[j]);
      return 1;
    }
  }
  // ---- the tiles whose distance range meets [edges[0], edges[last])
  const int64_t n_chrom = 2 * n;
  const int64_t nq = (n_chrom + 63) / 64;
  const int64_t pitch = (nq + LD_K - 1) / LD_K * LD_K;
  const int nt = (n_loci + 63) / 64;
  const double e_lo = edges[0], e_hi = edges[n_bins];
  auto first_of = [&](int t) { return pos[(size_t)t * 64]; };
  auto last_of = [&](int t) { return pos[std::min<size_t>((size_t)t * 64 + 63, (size_t)n_loci - 1)]; };
  // for an i-tile the listed j-tiles are a contiguous range (pos ascends): [jlo, jhi)
  std::vector<int32_t> jlo((size_t)nt), jhi((size_t)nt);
  int64_t n_listed = 0;
  for (int ti = 0; ti < nt; ++ti) {
    int lo = nt, hi = ti;
    for (int tj = ti; tj < nt; ++tj) {
      const double dmax = last_of(tj) - first_of(ti);
      const double dmin = tj == ti ? 0.0 : first_of(tj) - last_of(ti);
      if (!(dmin < e_hi)) break;
      if (dmax >= e_lo) {
        lo = std::min(lo, tj);
        hi = tj + 1;
      }
    }
    if (lo >= hi) lo = hi = ti;
    jlo[(size_t)ti] = lo;
    jhi[(size_t)ti] = hi;
    n_listed += hi - lo;
  }
  if ((long double)n_listed * (long double)nq >= 9223372036854775808.0L) {
    gnx_set_error("%s: the work leaves int64", who);
    return 1;
  }
  *work = n_listed * nq;
  if (max_work <= 0) return 0;
  if (*work > max_work) {
    gnx_set_error("%s: %lld tiles of 64 x 64 loci x %lld chromosome words = %lld tile-words of "
                  "work exceed max_work = %lld", who, (long long)n_listed, (long long)nq,
                  (long long)*work, (long long)max_work);
    return 1;
  }
  // ---- blocks of whole tiles: everything at once, or two blocks under the byte budget
  const int64_t budget = h->ld_budget > 0 ? h->ld_budget : LD_BUDGET;
  // (as allocated: whole tiles of rows padded to whole stages; one tile per block is the least,
  // also where two of them exceed the budget)
  int tpb = nt;
  if ((long double)nt * 64.0L * (long double)pitch * 8.0L > (long double)budget)
    tpb = (int)std::min<int64_t>(nt, std::max<int64_t>(1, budget / (2 * 64 * pitch * 8)));
  const int nblk = (nt + tpb - 1) / tpb;
  h->ld_blocks = nblk;
  // the genome lines (16 words) each block reads
  std::vector<int32_t> line_off((size_t)nblk + 1, 0), lines;
  for (int bk = 0; bk < nblk; ++bk) {
    const int ja = bk * tpb * 64, jb = std::min<int64_t>(n_loci, (int64_t)(bk + 1) * tpb * 64);
    std::vector<int32_t> ls;
    ls.reserve((size_t)(jb - ja));
    for (int j = ja; j < jb; ++j) ls.push_back(loci[j] >> 10);
    std::sort(ls.begin(), ls.end());
    ls.erase(std::unique(ls.begin(), ls.end()), ls.end());
    lines.insert(lines.end(), ls.begin(), ls.end());
    line_off[(size_t)bk + 1] = (int32_t)lines.size();
  }
  // the tasks of one launch at most
  int64_t max_tasks = 1;
  for (int bi = 0; bi < nblk; ++bi)
    for (int bj = bi; bj < nblk; ++bj) {
      int64_t m = 0;
      for (int ti = bi * tpb; ti < std::min(nt, (bi + 1) * tpb); ++ti)
        m += std::max(0, std::min<int>(jhi[(size_t)ti], std::min(nt, (bj + 1) * tpb)) -
                             std::max<int>(jlo[(size_t)ti], bj * tpb));
      max_tasks = std::max(max_tasks, m);
    }

  GnxScratch s(who);
  int32_t* d_rows = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows));
  const int64_t buf_words = (int64_t)tpb * 64 * pitch;
  u64 *TA = nullptr, *TB = nullptr;
  int32_t *d_jof = nullptr, *d_lines = nullptr;
  long long *d_c1 = nullptr, *d_ipart = nullptr, *d_itot = nullptr;
  double *d_pos = nullptr, *d_edges = nullptr, *d_fpart = nullptr, *d_ftot = nullptr;
  LdTask* d_tasks = nullptr;
  const int mf = LD_NB * LD_NF;
  GNXCHK(s.get(&TA, (size_t)buf_words));
  if (nblk > 1) GNXCHK(s.get(&TB, (size_t)buf_words));
  GNXCHK(s.get(&d_jof, jof.size()));
  GNXCHK(s.get(&d_lines, lines.size()));
  GNXCHK(s.get(&d_c1, (size_t)n_loci));
  GNXCHK(s.get(&d_pos, (size_t)n_loci));
  GNXCHK(s.get(&d_edges, (size_t)n_edges));
  GNXCHK(s.get(&d_tasks, (size_t)max_tasks));
  GNXCHK(s.get(&d_ipart, (size_t)LD_BLOCKS * LD_NB));
  GNXCHK(s.get(&d_fpart, (size_t)LD_BLOCKS * mf));
  GNXCHK(s.get(&d_itot, (size_t)LD_NB));
  GNXCHK(s.get(&d_ftot, (size_t)mf));
  GNXCHK(gnx_h2d(h, d_jof, jof.data(), jof.size() * sizeof(int32_t)));
  GNXCHK(gnx_h2d(h, d_lines, lines.data(), lines.size() * sizeof(int32_t)));
  GNXCHK(gnx_h2d(h, d_pos, pos, (size_t)n_loci * sizeof(double)));
  GNXCHK(gnx_h2d(h, d_edges, edges, (size_t)n_edges * sizeof(double)));
  HIPCHK(hipMemsetAsync(d_itot, 0, LD_NB * sizeof(long long), h->stream));
  HIPCHK(hipMemsetAsync(d_ftot, 0, mf * sizeof(double), h->stream));
  HIPCHK(hipMemsetAsync(d_c1, 0, (size_t)n_loci * sizeof(long long), h->stream));

  std::vector<bool> counted((size_t)nblk, false);
  // block bk into buf (rows past the block and words past the sample: 0), and its c1 the first
  // time; -> kernels launched
  auto transpose = [&](int bk, u64* buf) -> int {
    const int ja = bk * tpb * 64;
    const int nj = (int)std::min<int64_t>(n_loci - ja, (int64_t)tpb * 64);
    const bool first = !counted[(size_t)bk];
    counted[(size_t)bk] = true;
    return ld_transpose(h, n_chrom, nq, pitch, line_off[(size_t)bk + 1] - line_off[(size_t)bk],
                        d_lines + line_off[(size_t)bk], d_rows, d_jof, ja, nj, buf, buf_words,
                        first ? d_c1 + ja : nullptr);
  };
  const long long mm = std::max<long long>(1, min_minor);
  std::vector<LdTask> tasks;
  GnxCallTimer tm(h, &h->ld_ms, &h->ld_launches);
  for (int bi = 0; bi < nblk; ++bi) {
    bool have_a = false;
    for (int bj = bi; bj < nblk; ++bj) {
      tasks.clear();
      const int tj0 = bj * tpb, tj1 = std::min(nt, (bj + 1) * tpb);
      for (int ti = bi * tpb; ti < std::min(nt, (bi + 1) * tpb); ++ti)
        for (int tj = std::max<int>(jlo[(size_t)ti], tj0); tj < std::min<int>(jhi[(size_t)ti], tj1);
             ++tj)
          tasks.push_back(LdTask{ti, tj});
      // (block bi is transposed even without a task of its own: its c1 is an output)
      if (tasks.empty() && bj > bi) continue;
      if (!tasks.empty())
        GNXCHK(gnx_h2d(h, d_tasks, tasks.data(), tasks.size() * sizeof(LdTask)));
      int64_t launches = 0;
      tm.start();
      if (!have_a) {
        launches += transpose(bi, TA);
        have_a = true;
      }
      if (bj > bi) launches += transpose(bj, TB);
      if (!tasks.empty()) {
        const int blocks = (int)std::min<int64_t>((int64_t)tasks.size(), LD_BLOCKS);
        hipLaunchKernelGGL(k_ld_pairs, dim3(blocks), dim3(256), 0, h->stream,
                           (int64_t)tasks.size(), d_tasks, pitch, (int)n_loci, TA, bi * tpb,
                           bj > bi ? TB : TA, bj * tpb, (long long)n_chrom, mm, (int)(morgans != 0),
                           n_bins, d_c1, d_pos, d_edges, d_ipart, d_fpart);
        hipLaunchKernelGGL(k_ld_total, dim3(gnx_grid(LD_NB + mf, 256)), dim3(256), 0, h->stream,
                           blocks, d_ipart, d_fpart, d_itot, d_ftot);
        launches += 2;
      }
      HIPCHK(hipGetLastError());
      GNXCHK(tm.stop(launches));
    }
  }
  std::vector<long long> itot((size_t)LD_NB), c1h((size_t)n_loci);
  std::vector<double> ftot((size_t)mf);
  GNXCHK(gnx_d2h(h, itot.data(), d_itot, itot.size() * sizeof(long long)));
  GNXCHK(gnx_d2h(h, ftot.data(), d_ftot, ftot.size() * sizeof(double)));
  GNXCHK(gnx_d2h(h, c1h.data(), d_c1, c1h.size() * sizeof(long long)));
  for (int j = 0; j < n_loci; ++j) c1[j] = c1h[(size_t)j];
  for (int k = 0; k < n_bins; ++k) {
    pairs[k] = itot[(size_t)k];
    for (int q = 0; q < LD_NF; ++q) fsums[k * LD_NF + q] = ftot[(size_t)k * LD_NF + q];
  }
  return 0;
}
