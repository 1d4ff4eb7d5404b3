// Fine-scale spatial genetic structure on the device: the sums over the pairs of individuals
// closer than the largest distance class from which mean kinship per class, its slope on
// ln(distance), Sp and the neighbourhood size follow by fp64 algebra on the host
// (geonomics_amd/sim/sgs.py).  No n x n matrix: only the pairs of individuals in the same or
// adjacent cells of a grid whose side is at least the largest edge are looked at, so the call
// works on the whole population.  (The reference has no such analysis: its IBD demo,
// demos/_IBD_IBE.py, ends at MMRR on a sample.)
//
//   gnx_sgs_sums   isums [n_bins][3] exact int64, fsums [n_bins][7] fp64, n_zero
//
// The sample is sorted by cell (gnx_prim_sort on the cell number, stable), and the packed
// dosage operand is gathered in that order (k_geno_gather through the block tables, and through
// `perm` where given), so the rows of a cell are contiguous.  k_sgs_self takes, per row, self =
// sum d^2 (popcounts) and w = sum weight[l] d_l (fp64, loci ascending).  The host reads the
// cells' row ranges back (one int32 per cell), counts the candidate pairs - the work limit is
// checked here, before the operand is even allocated - and lists the tasks: a 64 x 64 tile of
// rows of (cell, cell) or of (cell, one of its four forward neighbours).
//
// k_sgs_pairs: a fixed grid of workgroups, workgroup g takes tasks g, g + grid, ...  The body of
// a task is the popcount tile of k_geno_gram (geno_tile64 with geno_dot16, gnx_geno.h: thread
// (tx, ty) owns rows ty + 16 r and columns tx + 16 c).  The epilogue takes the thread's four
// rows one at a time (all 16 pairs at once take more than 256 registers): r, the
// class and ln r of the row's four pairs (a diagonal tile of a cell with itself keeps i < j),
// then, for every class present in the wave, each lane adds its own pairs' ten terms, the wave
// adds its lanes by an xor butterfly and lane 0 adds the result to the wave's accumulators in LDS.  A workgroup
// leaves one partial (its four waves added in wave order); k_sgs_total adds the partials in
// workgroup order.  No atomics: every sum is taken in an order fixed by (n, cells, n_bins), so
// the fp64 sums of a call repeated are bit-equal too.
#include "gnx_sgs.h"

#define SGS_NB 32            // distance classes at most
#define SGS_NI 3             // integer sums per class
#define SGS_NF 7             // fp64 sums per class
#define SGS_BLOCKS 1024      // workgroups of the pair kernel at most (one partial each)

// key[i] = the cell of sample index i, val[i] = i
__global__ void k_sgs_cells(int64_t n, const int64_t* __restrict__ slots,
                            const float* __restrict__ x, const float* __restrict__ y, double side,
                            int ncx, int ncy, uint32_t* __restrict__ key,
                            int32_t* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t s = slots ? slots[i] : i;
  double cx = floor((double)x[s] / side), cy = floor((double)y[s] / side);
  // clamped (coordinates on or past the border, NaN): clamping keeps neighbours neighbours
  if (!(cx >= 0.0)) cx = 0.0;
  if (!(cy >= 0.0)) cy = 0.0;
  if (cx > (double)(ncx - 1)) cx = (double)(ncx - 1);
  if (cy > (double)(ncy - 1)) cy = (double)(ncy - 1);
  key[i] = (uint32_t)((int)cy * ncx + (int)cx);
  val[i] = (int32_t)i;
}

// start[c] = the first sorted position whose cell is >= c (c = 0 .. n_cells)
__global__ void k_sgs_cell_start(int64_t n, int n_cells, const uint32_t* __restrict__ key,
                                 int32_t* __restrict__ start) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > n_cells) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (key[mid] < (uint32_t)c) lo = mid + 1;
    else hi = mid;
  }
  start[c] = (int32_t)lo;
}

// sorted position j holds sample index o = order[j]: its own coordinates, and the genome row of
// sample index perm[o]
__global__ void k_sgs_arrange(int64_t n, const int32_t* __restrict__ order,
                              const int64_t* __restrict__ slots, const int32_t* __restrict__ perm,
                              const int32_t* __restrict__ rows, const float* __restrict__ x,
                              const float* __restrict__ y, int32_t* __restrict__ rows_sorted,
                              float* __restrict__ xs, float* __restrict__ ys) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int32_t o = order[j];
  const int64_t s = slots ? slots[o] : o;
  rows_sorted[j] = rows[perm ? perm[o] : o];
  xs[j] = x[s];
  ys[j] = y[s];
}

// self[i] = sum over the masked loci of d^2, w[i] = sum of weight[l] d_l in ascending l (fp64;
// weight[l] d is exact, so each step rounds once, as numpy's does); weight == null: w = 0
__global__ void k_sgs_self(int64_t n, int nw, int Wm, const u64* __restrict__ X,
                           const int32_t* __restrict__ widx, const double* __restrict__ weight,
                           int32_t* __restrict__ self, double* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64* a = X + (i * 2) * Wm;
  const u64* b = a + Wm;
  int s = 0;
  double acc = 0.0;
  for (int q = 0; q < nw; ++q) {
    const u64 av = a[q], bv = b[q];
    s += __popcll(av) + __popcll(bv) + 2 * __popcll(av & bv);
    if (weight) {
      const double* wl = weight + (int64_t)widx[q] * 64;
      for (u64 m = av | bv; m; m &= m - 1) {
        const int bit = __ffsll((long long)m) - 1;
        acc += wl[bit] * (double)((int)((av >> bit) & 1ull) + (int)((bv >> bit) & 1ull));
      }
    }
  }
  self[i] = s;
  w[i] = acc;
}

__device__ __forceinline__ double sgs_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ long long sgs_wave_sum(long long v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// ipart[g][SGS_NB + 1][SGS_NI]: class k = {pairs, sum dot, sum (self_a + self_b)}, row SGS_NB =
// {pairs with r == 0, -, -};  fpart[g][SGS_NB][SGS_NF] = {sum r, sum ln r, sum ln^2 r,
// sum dot ln r, sum (self_a + self_b) ln r, sum (w_a + w_b), sum (w_a + w_b) ln r}
__global__ void __launch_bounds__(256)
k_sgs_pairs(int64_t n_tasks, int Wm, int n_bins, const SgsTask* __restrict__ tasks,
            const u64* __restrict__ X, const float* __restrict__ xs,
            const float* __restrict__ ys, const int32_t* __restrict__ self,
            const double* __restrict__ w, const double* __restrict__ edges,
            long long* __restrict__ ipart, double* __restrict__ fpart) {
  __shared__ GenoStage S;
  __shared__ double E[SGS_NB + 1];
  __shared__ float cx[2][64], cy[2][64];
  __shared__ int32_t cs[2][64];
  __shared__ double cw[2][64];
  __shared__ long long Iw[4][SGS_NB + 1][SGS_NI];
  __shared__ double Fw[4][SGS_NB][SGS_NF];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, wave = tid >> 6, lane = tid & 63;
  for (int q = tid; q < 4 * (SGS_NB + 1) * SGS_NI; q += 256) (&Iw[0][0][0])[q] = 0;
  for (int q = tid; q < 4 * SGS_NB * SGS_NF; q += 256) (&Fw[0][0][0])[q] = 0.0;
  if (tid <= n_bins) E[tid] = edges[tid];
  for (int64_t t = blockIdx.x; t < n_tasks; t += gridDim.x) {
    const SgsTask T = tasks[t];
    __syncthreads();                                // the last task's epilogue has read c*
    if (tid < 128) {
      const int side = tid >> 6, i = tid & 63;
      const int64_t row = (side ? T.b0 : T.a0) + i;
      const bool live = i < (side ? T.nb : T.na);
      cx[side][i] = live ? xs[row] : 0.f;
      cy[side][i] = live ? ys[row] : 0.f;
      cs[side][i] = live ? self[row] : 0;
      cw[side][i] = live ? w[row] : 0.0;
    }
    int acc[4][4] = {};
    geno_tile64(S, X, Wm, T.a0, T.b0, [&](auto& ai, auto& bi, auto& aj, auto& bj) {
      geno_dot16(acc, ai, bi, aj, bj);
    });
    // ---- epilogue, one of the thread's four rows (four pairs) at a time: r, class, ln r
    const bool diag = T.a0 == T.b0;
    long long nz = 0;
#pragma unroll 1
    for (int r = 0; r < 4; ++r) {                   // (one copy of the body)
      const int i = ty + 16 * r;
      const double xa = (double)cx[0][i], ya = (double)cy[0][i], wa = cw[0][i];
      const int sa = cs[0][i];
      double rad[4], lnr[4], ww[4];
      int ss[4], bin[4], dots[4];
      unsigned present = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        dots[c] = r == 0 ? acc[0][c] : r == 1 ? acc[1][c] : r == 2 ? acc[2][c] : acc[3][c];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = tx + 16 * c;
        const double dx = xa - (double)cx[1][j], dy = ya - (double)cy[1][j];
        const double d = sqrt(dx * dx + dy * dy);
        int b = -1;
        if (i < T.na && j < T.nb && (!diag || i < j)) {
          if (d == 0.0) ++nz;
          else if (d >= E[0] && d < E[n_bins]) {
            int lo = 0, hi = n_bins;
            while (hi - lo > 1) {
              const int mid = (lo + hi) >> 1;
              if (d >= E[mid]) lo = mid;
              else hi = mid;
            }
            b = lo;
          }
        }
        bin[c] = b;
        rad[c] = d;
        lnr[c] = b >= 0 ? log(d) : 0.0;
        ss[c] = sa + cs[1][j];
        ww[c] = wa + cw[1][j];
        if (b >= 0) present |= 1u << b;
      }
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) present |= (unsigned)__shfl_xor((int)present, d, 64);
      present = (unsigned)__builtin_amdgcn_readfirstlane((int)present);
      while (present) {                             // wave-uniform: the classes in the wave
        const int k = __ffs((int)present) - 1;
        present &= present - 1;
        long long ic = 0, id = 0, is = 0;
        double f[SGS_NF];
#pragma unroll
        for (int q = 0; q < SGS_NF; ++q) f[q] = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (bin[c] == k) {
            const double dot = (double)dots[c], l = lnr[c];
            ic += 1;
            id += dots[c];
            is += ss[c];
            f[0] += rad[c];
            f[1] += l;
            f[2] += l * l;
            f[3] += dot * l;
            f[4] += (double)ss[c] * l;
            f[5] += ww[c];
            f[6] += ww[c] * l;
          }
        ic = sgs_wave_sum(ic);
        id = sgs_wave_sum(id);
        is = sgs_wave_sum(is);
#pragma unroll
        for (int q = 0; q < SGS_NF; ++q) f[q] = sgs_wave_sum(f[q]);
        if (lane == 0) {
          Iw[wave][k][0] += ic;
          Iw[wave][k][1] += id;
          Iw[wave][k][2] += is;
#pragma unroll
          for (int q = 0; q < SGS_NF; ++q) Fw[wave][k][q] += f[q];
        }
      }
    }
    nz = sgs_wave_sum(nz);
    if (lane == 0) Iw[wave][SGS_NB][0] += nz;
  }
  __syncthreads();
  for (int q = tid; q < (SGS_NB + 1) * SGS_NI; q += 256) {
    const long long* p = &Iw[0][0][0] + q;
    const int m = (SGS_NB + 1) * SGS_NI;
    ipart[(int64_t)blockIdx.x * m + q] = p[0] + p[m] + p[2 * m] + p[3 * m];
  }
  for (int q = tid; q < SGS_NB * SGS_NF; q += 256) {
    const double* p = &Fw[0][0][0] + q;
    const int m = SGS_NB * SGS_NF;
    fpart[(int64_t)blockIdx.x * m + q] = ((p[0] + p[m]) + p[2 * m]) + p[3 * m];
  }
}

// the workgroups' partials added in workgroup order
__global__ void k_sgs_total(int blocks, const long long* __restrict__ ipart,
                            const double* __restrict__ fpart, long long* __restrict__ itot,
                            double* __restrict__ ftot) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int mi = (SGS_NB + 1) * SGS_NI, mf = SGS_NB * SGS_NF;
  if (q < mi) {
    long long s = 0;
    for (int g = 0; g < blocks; ++g) s += ipart[(int64_t)g * mi + q];
    itot[q] = s;
  } else if (q < mi + mf) {
    const int c = q - mi;
    double s = 0.0;
    for (int g = 0; g < blocks; ++g) s += fpart[(int64_t)g * mf + c];
    ftot[c] = s;
  }
}

extern "C" int gnx_sgs_sums(gnx_state* h, int64_t n, const int64_t* slots,
                            const uint64_t* locus_mask, int32_t n_bins, const double* edges,
                            const double* locus_weight, const int32_t* perm, int64_t max_work,
                            int64_t* work, int64_t* isums, double* fsums, int64_t* n_zero) {
  const char* who = "gnx_sgs_sums";
  GNXCHK(geno_ready(h, who));
  if (n < 1 || n > (1ll << 24)) {
    gnx_set_error("%s: 1..2^24 individuals per call (got %lld)", who, (long long)n);
    return 1;
  }
  if (n_bins < 1 || n_bins > SGS_NB) {
    gnx_set_error("%s: 1..%d distance classes (got %d)", who, SGS_NB, n_bins);
    return 1;
  }
  if (!edges || !work || (max_work > 0 && (!isums || !fsums || !n_zero))) {
    gnx_set_error("%s: null edges, work or output", who);
    return 1;
  }
  for (int k = 0; k <= n_bins; ++k)
    if (!std::isfinite(edges[k]) || edges[k] < 0.0 || (k > 0 && !(edges[k] > edges[k - 1]))) {
      gnx_set_error("%s: edges must be finite, ascending and start at or above 0 (edges[%d] = %g)",
                    who, k, edges[k]);
      return 1;
    }
  for (int64_t i = 0; perm && i < n; ++i)
    if (perm[i] < 0 || perm[i] >= n) {
      gnx_set_error("%s: perm[%lld] = %d is not in 0..n-1", who, (long long)i, perm[i]);
      return 1;
    }
  const int L = h->cfg.L;
  // an isums entry is at most pairs * 8 L (self_a + self_b <= 8 L)
  if ((long double)n * (long double)(n - 1) / 2.0L * 8.0L * (long double)L >=
      9223372036854775808.0L) {
    gnx_set_error("%s: %lld individuals x %d loci: an integer sum could leave int64", who,
                  (long long)n, L);
    return 1;
  }
  std::vector<int32_t> widx;
  std::vector<u64> wmask;
  geno_words(h, locus_mask, widx, wmask);
  const int nw = (int)widx.size();
  // the grid: its side is just above the largest edge
  const SgsGrid grid = sgs_grid(h, edges[n_bins]);

  GnxScratch s(who);
  int32_t* d_rows = nullptr;
  int64_t* d_slots = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows, &d_slots));
  const GnxSoA a = h->soa[h->cur];
  int32_t *d_order = nullptr, *d_perm = nullptr;
  std::vector<int32_t> start;
  GNXCHK(sgs_sort_cells(h, s, grid, n, d_slots, &d_order, start));
  // the candidate pairs: a cell with itself and with its four forward neighbours
  int64_t cand = 0, n_tasks = 0;
  sgs_count_pairs(grid, start, &cand, &n_tasks);
  *work = cand * (int64_t)nw;
  if (max_work <= 0) return 0;
  if (*work > max_work) {
    gnx_set_error("%s: %lld candidate pairs x %d words = %lld pair-words of work exceed "
                  "max_work = %lld", who, (long long)cand, nw, (long long)*work,
                  (long long)max_work);
    return 1;
  }
  std::vector<SgsTask> tasks;
  sgs_list_tasks(grid, start, n_tasks, tasks);
  n_tasks = (int64_t)tasks.size();
  const int blocks = (int)std::min<int64_t>(std::max<int64_t>(n_tasks, 1), SGS_BLOCKS);
  const int mi = (SGS_NB + 1) * SGS_NI, mf = SGS_NB * SGS_NF;
  // a tile reads 64 rows from its first: 64 zero rows behind the sample
  const int64_t n_pad = n + 64;
  int32_t *d_rows_sorted = nullptr, *d_self = nullptr;
  float *d_xs = nullptr, *d_ys = nullptr;
  double *d_w = nullptr, *d_weight = nullptr, *d_edges = nullptr, *d_fpart = nullptr,
         *d_ftot = nullptr;
  long long *d_ipart = nullptr, *d_itot = nullptr;
  SgsTask* d_tasks = nullptr;
  GNXCHK(s.get(&d_rows_sorted, (size_t)n));
  GNXCHK(s.get(&d_xs, (size_t)n));
  GNXCHK(s.get(&d_ys, (size_t)n));
  GNXCHK(s.get(&d_self, (size_t)n));
  GNXCHK(s.get(&d_w, (size_t)n));
  GNXCHK(s.get(&d_edges, (size_t)n_bins + 1));
  GNXCHK(s.get(&d_tasks, (size_t)n_tasks));
  GNXCHK(s.get(&d_ipart, (size_t)blocks * mi));
  GNXCHK(s.get(&d_fpart, (size_t)blocks * mf));
  GNXCHK(s.get(&d_itot, (size_t)mi));
  GNXCHK(s.get(&d_ftot, (size_t)mf));
  if (perm) {
    GNXCHK(s.get(&d_perm, (size_t)n));
    GNXCHK(gnx_h2d(h, d_perm, perm, (size_t)n * sizeof(int32_t)));
  }
  if (locus_weight) {
    // padded to whole words: k_sgs_self indexes it by word * 64 + bit
    std::vector<double> wt((size_t)h->W64 * 64, 0.0);
    std::copy(locus_weight, locus_weight + L, wt.begin());
    GNXCHK(s.get(&d_weight, wt.size()));
    GNXCHK(gnx_h2d(h, d_weight, wt.data(), wt.size() * sizeof(double)));
  }
  GNXCHK(gnx_h2d(h, d_edges, edges, ((size_t)n_bins + 1) * sizeof(double)));
  if (n_tasks) GNXCHK(gnx_h2d(h, d_tasks, tasks.data(), (size_t)n_tasks * sizeof(SgsTask)));
  hipLaunchKernelGGL(k_sgs_arrange, dim3(gnx_grid(n, 256)), dim3(256), 0, h->stream, n, d_order,
                     d_slots, d_perm, d_rows, a.x, a.y, d_rows_sorted, d_xs, d_ys);
  GenoOperand op;
  GNXCHK(geno_operand(h, s, n_pad, widx, wmask, 0, &op));
  geno_gather(h, d_rows_sorted, n, op);
  hipLaunchKernelGGL(k_sgs_self, dim3(gnx_grid(n, 64)), dim3(64), 0, h->stream, n, nw, op.Wm,
                     op.X, op.widx, d_weight, d_self, d_w);
  hipLaunchKernelGGL(k_sgs_pairs, dim3(blocks), dim3(256), 0, h->stream, n_tasks, op.Wm,
                     (int)n_bins, d_tasks, op.X, d_xs, d_ys, d_self, d_w, d_edges, d_ipart,
                     d_fpart);
  hipLaunchKernelGGL(k_sgs_total, dim3(gnx_grid(mi + mf, 256)), dim3(256), 0, h->stream, blocks,
                     d_ipart, d_fpart, d_itot, d_ftot);
  HIPCHK(hipGetLastError());
  std::vector<long long> itot((size_t)mi);
  std::vector<double> ftot((size_t)mf);
  GNXCHK(gnx_d2h(h, itot.data(), d_itot, itot.size() * sizeof(long long)));
  GNXCHK(gnx_d2h(h, ftot.data(), d_ftot, ftot.size() * sizeof(double)));
  for (int k = 0; k < n_bins; ++k) {
    for (int q = 0; q < SGS_NI; ++q) isums[k * SGS_NI + q] = itot[(size_t)k * SGS_NI + q];
    for (int q = 0; q < SGS_NF; ++q) fsums[k * SGS_NF + q] = ftot[(size_t)k * SGS_NF + q];
  }
  *n_zero = itot[(size_t)SGS_NB * SGS_NI];
  return 0;
}
