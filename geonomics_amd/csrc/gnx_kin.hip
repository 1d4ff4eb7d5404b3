// Close-kin pairs on the device: who is related to whom (the reference has no such analysis).
// KING-robust kinship (Manichaikul et al. 2010) needs two integers per pair of individuals, the
// loci at which both are heterozygous (hh) and those at which they are opposite homozygotes
// (ibs0), and one per individual (nhet); the kinship itself is fp64 algebra on the host
// (geonomics_amd/sim/kin.py).  include/gnx_hip.h has the definitions.
//
//   gnx_kin_matrix   nhet [n], hh [n][n], ibs0 [n][n] int32, n <= 8192
//   gnx_kin_pairs    the pairs closer than max_dist whose kinship reaches a threshold, as a list
//                    sorted by (pa, pb): no n x n matrix, n <= 2^24
//   gnx_kin_info     kernel time, launches and tiles of the last call
//
// The operand is the gathered X [rows][2][words] of the Gram kernel (gnx_geno.h): masked and
// padded bits are 0 in both homologues.  Per row and word, in registers, het = a0 ^ a1,
// P = a0 & a1 (homozygous 1) and N = ~(a0 | a1); per pair and word three popcounts,
// hh += pc(het_a & het_b), ibs0 += pc(P_a & N_b) + pc(P_b & N_a).  N is 1 at the masked bits,
// but P is 0 there, so they add nothing.  (A gather that wrote het, P, N instead would save the
// six logic operations per row and word, which the 16 pairs of a thread share, and cost half as
// much operand again: derived in registers)
//
// kin_tile is the LDS-staged 64 x 64 popcount tile of k_geno_gram (stages of GRAM_GK words,
// thread (tx, ty) owns rows ty + 16 r and columns tx + 16 c) with two int accumulators per
// pair.  k_kin_matrix takes one tile of the upper triangle per workgroup and mirrors it.
// k_kin_pairs follows k_sgs_pairs: the sample sorted by cell, the host's list of tiles over the
// pairs of rows of the same or adjacent cells (gnx_sgs.h), a fixed grid of workgroups striding
// over the tasks.  Its epilogue takes the thread's four rows one at a time: r in fp64 from the
// fp32 coordinates, the integer keep rule, a ballot of the keepers per column, ONE atomicAdd per
// wave on the list counter for the row's keepers, and each keeper written at the base plus its
// rank in the ballots.  Past the list's capacity keepers are counted, not written.  The list
// arrives in an order that depends on the schedule; its entries are integers and its 64-bit keys
// pa * n + pb are distinct, so sorting by key (gnx_prim_sort64) makes the output of a repeated
// call byte-equal.
#include "gnx_sgs.h"

#define KIN_BLOCKS 1024      // workgroups of the pair kernel at most
#define KIN_SHIFT 20         // the threshold is T / 2^20

// nh[j] = the heterozygous loci of operand row j; with order, also by_sample[order[j]] = nh[j]
__global__ void k_kin_nhet(int64_t n, int nw, int Wm, const u64* __restrict__ X,
                           const int32_t* __restrict__ order, int32_t* __restrict__ nh,
                           int32_t* __restrict__ by_sample) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const u64* a = X + (j * 2) * Wm;
  const u64* b = a + Wm;
  int s = 0;
  for (int q = 0; q < nw; ++q) s += __popcll(a[q] ^ b[q]);
  nh[j] = s;
  if (order) by_sample[order[j]] = s;
}

// hh[r][c], ib[r][c] of rows a0 + ty + 16 r against rows b0 + tx + 16 c of X over all Wm words
__device__ __forceinline__ void kin_tile(const u64* __restrict__ X, int Wm, int64_t a0, int64_t b0,
                                         int (&hh)[4][4], int (&ib)[4][4]) {
  __shared__ u64 As[GRAM_GK][2][64];
  __shared__ u64 Bs[GRAM_GK][2][64];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) hh[r][c] = ib[r][c] = 0;
  for (int k0 = 0; k0 < Wm; k0 += GRAM_GK) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int q = tid + 256 * s;                    // (row, hom, word) with the word fastest
      const int row = q >> 5, hom = (q >> 4) & 1, kk = q & 15;
      As[kk][hom][row] = X[((a0 + row) * 2 + hom) * Wm + k0 + kk];
      Bs[kk][hom][row] = X[((b0 + row) * 2 + hom) * Wm + k0 + kk];
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < GRAM_GK; ++kk) {
      u64 ha[4], pa[4], na[4], hb[4], pb[4], nb[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const u64 a0w = As[kk][0][ty + 16 * r], a1w = As[kk][1][ty + 16 * r];
        const u64 b0w = Bs[kk][0][tx + 16 * r], b1w = Bs[kk][1][tx + 16 * r];
        ha[r] = a0w ^ a1w;
        pa[r] = a0w & a1w;
        na[r] = ~(a0w | a1w);
        hb[r] = b0w ^ b1w;
        pb[r] = b0w & b1w;
        nb[r] = ~(b0w | b1w);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          hh[r][c] += __popcll(ha[r] & hb[c]);
          ib[r][c] += __popcll(pa[r] & nb[c]) + __popcll(pb[c] & na[r]);
        }
    }
    __syncthreads();
  }
}

// one 64 x 64 tile per block (upper triangle of tiles only, mirrored on the write)
__global__ void __launch_bounds__(256)
k_kin_matrix(int64_t n, int Wm, const u64* __restrict__ X, int32_t* __restrict__ hh_out,
             int32_t* __restrict__ ib_out) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj < ti) return;                              // block-uniform
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t i0 = (int64_t)ti * 64, j0 = (int64_t)tj * 64;
  int hh[4][4], ib[4][4];
  kin_tile(X, Wm, i0, j0, hh, ib);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
      if (i < n && j < n) {
        hh_out[i * n + j] = hh[r][c];
        hh_out[j * n + i] = hh[r][c];
        ib_out[i * n + j] = ib[r][c];
        ib_out[j * n + i] = ib[r][c];
      }
    }
}

// counters[0]: the keepers (all of them, written or not), counters[1]: the candidates.
// key[k] = pa * n + pb (sample indices, pa < pb), lhh[k], lib[k]: keeper k < cap, in any order
__global__ void __launch_bounds__(256)
k_kin_pairs(int64_t n_tasks, int Wm, int64_t n, const SgsTask* __restrict__ tasks,
            const u64* __restrict__ X, const float* __restrict__ xs,
            const float* __restrict__ ys, const int32_t* __restrict__ nh,
            const int32_t* __restrict__ order, int all, double max_dist, long long T,
            unsigned long long cap, unsigned long long* __restrict__ counters,
            u64* __restrict__ key, int32_t* __restrict__ lhh, int32_t* __restrict__ lib) {
  __shared__ float cx[2][64], cy[2][64];
  __shared__ int32_t cn[2][64], co[2][64];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63;
  const u64 below = (1ull << lane) - 1ull;
  unsigned long long n_cand = 0;
  for (int64_t t = blockIdx.x; t < n_tasks; t += gridDim.x) {
    const SgsTask K = tasks[t];
    __syncthreads();                                // the last task's epilogue has read c*
    if (tid < 128) {
      const int side = tid >> 6, i = tid & 63;
      const int64_t row = (side ? K.b0 : K.a0) + i;
      const bool live = i < (side ? K.nb : K.na);
      cx[side][i] = live ? xs[row] : 0.f;
      cy[side][i] = live ? ys[row] : 0.f;
      cn[side][i] = live ? nh[row] : 0;
      co[side][i] = live ? order[row] : 0;
    }
    int hh[4][4], ib[4][4];
    kin_tile(X, Wm, K.a0, K.b0, hh, ib);            // (its barriers publish c* too)
    // ---- epilogue, one of the thread's four rows (four pairs) at a time
    const bool diag = K.a0 == K.b0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = ty + 16 * r;
      const double xa = (double)cx[0][i], ya = (double)cy[0][i];
      const long long na = cn[0][i];
      const long long oa = co[0][i];
      bool keep[4];
      u64 bal[4];
      int total = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = tx + 16 * c;
        const double dx = xa - (double)cx[1][j], dy = ya - (double)cy[1][j];
        const double d = sqrt(dx * dx + dy * dy);
        const bool cand = i < K.na && j < K.nb && (!diag || i < j) && (all || d < max_dist);
        const long long den = na + cn[1][j];
        const long long num = (long long)hh[r][c] - 2ll * ib[r][c];
        n_cand += cand ? 1ull : 0ull;
        keep[c] = cand && den > 0 && num * (1ll << KIN_SHIFT) >= T * den;
        bal[c] = __ballot(keep[c]);
        total += __popcll(bal[c]);
      }
      if (total == 0) continue;                     // wave-uniform
      unsigned long long base = 0;
      if (lane == 0) base = atomicAdd(&counters[0], (unsigned long long)total);
      base = (unsigned long long)__shfl((long long)base, 0, 64);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const unsigned long long k = base + (unsigned long long)__popcll(bal[c] & below);
        if (keep[c] && k < cap) {
          const long long ob = co[1][tx + 16 * c];
          const long long lo = oa < ob ? oa : ob, hi = oa < ob ? ob : oa;
          key[k] = (u64)(lo * n + hi);
          lhh[k] = hh[r][c];
          lib[k] = ib[r][c];
        }
        base += (unsigned long long)__popcll(bal[c]);
      }
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) n_cand += (unsigned long long)__shfl_xor((long long)n_cand, d, 64);
  if (lane == 0 && n_cand) atomicAdd(&counters[1], n_cand);
}

// the sorted list: entry k is (key[k] / n, key[k] % n) with the integers of list entry src[k]
__global__ void k_kin_emit(int64_t m, int64_t n, const u64* __restrict__ key,
                           const int32_t* __restrict__ src, const int32_t* __restrict__ lhh,
                           const int32_t* __restrict__ lib, int32_t* __restrict__ pa,
                           int32_t* __restrict__ pb, int32_t* __restrict__ hh,
                           int32_t* __restrict__ ib) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const u64 a = key[k] / (u64)n;
  pa[k] = (int32_t)a;
  pb[k] = (int32_t)(key[k] - a * (u64)n);
  hh[k] = lhh[src[k]];
  ib[k] = lib[src[k]];
}

__global__ void k_kin_iota(int64_t m, int32_t* __restrict__ v) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < m) v[k] = (int32_t)k;
}

extern "C" int gnx_kin_info(gnx_state* h, double* kernel_ms, int64_t* launches, int64_t* tasks) {
  if (kernel_ms) *kernel_ms = h->kin_ms;
  if (launches) *launches = h->kin_launches;
  if (tasks) *tasks = h->kin_tasks;
  return 0;
}

extern "C" int gnx_kin_matrix(gnx_state* h, int64_t n, const int64_t* slots,
                              const uint64_t* locus_mask, int32_t* nhet, int32_t* hh,
                              int32_t* ibs0) {
  const char* who = "gnx_kin_matrix";
  GNXCHK(geno_ready(h, who));
  if (n < 1 || n > 8192) {
    gnx_set_error("%s: 1..8192 individuals per call (the matrices are n x n)", who);
    return 1;
  }
  if (!nhet || !hh || !ibs0) {
    gnx_set_error("%s: null output", who);
    return 1;
  }
  h->kin_ms = 0.0;
  h->kin_launches = h->kin_tasks = 0;
  GnxScratch s(who);
  int32_t* d_rows = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows));
  std::vector<int32_t> widx;
  std::vector<u64> wmask;
  geno_words(h, locus_mask, widx, wmask);
  const int64_t n_pad = (n + 63) / 64 * 64;
  const int T = (int)(n_pad / 64);
  GenoOperand op;
  GNXCHK(geno_operand(h, s, n_pad, widx, wmask, 0, &op));
  int32_t *d_nh = nullptr, *d_hh = nullptr, *d_ib = nullptr;
  GNXCHK(s.get(&d_nh, (size_t)n));
  GNXCHK(s.get(&d_hh, (size_t)n * n));
  GNXCHK(s.get(&d_ib, (size_t)n * n));
  GnxCallTimer tm(h, &h->kin_ms, &h->kin_launches);
  tm.start();
  geno_gather(h, d_rows, n, op);
  hipLaunchKernelGGL(k_kin_nhet, dim3(gnx_grid(n, 64)), dim3(64), 0, h->stream, n, op.nw, op.Wm,
                     op.X, (const int32_t*)nullptr, d_nh, (int32_t*)nullptr);
  hipLaunchKernelGGL(k_kin_matrix, dim3(T, T), dim3(256), 0, h->stream, n, op.Wm, op.X, d_hh,
                     d_ib);
  HIPCHK(hipGetLastError());
  GNXCHK(tm.stop(3));
  h->kin_tasks = (int64_t)T * (T + 1) / 2;
  GNXCHK(gnx_d2h(h, nhet, d_nh, (size_t)n * sizeof(int32_t)));
  GNXCHK(gnx_d2h(h, hh, d_hh, (size_t)n * n * sizeof(int32_t)));
  return gnx_d2h(h, ibs0, d_ib, (size_t)n * n * sizeof(int32_t));
}

extern "C" int gnx_kin_pairs(gnx_state* h, int64_t n, const int64_t* slots,
                             const uint64_t* locus_mask, double max_dist, int64_t T,
                             int64_t max_pairs, int64_t max_work, int64_t* work,
                             int64_t* n_candidates, int64_t* n_found, int32_t* pa, int32_t* pb,
                             int32_t* hh, int32_t* ibs0, int32_t* nhet) {
  const char* who = "gnx_kin_pairs";
  GNXCHK(geno_ready(h, who));
  if (n < 1 || n > (1ll << 24)) {
    gnx_set_error("%s: 1..2^24 individuals per call (got %lld)", who, (long long)n);
    return 1;
  }
  if (std::isnan(max_dist)) {
    gnx_set_error("%s: max_dist is NaN", who);
    return 1;
  }
  if (T < -(1ll << KIN_SHIFT) || T > (1ll << (KIN_SHIFT - 1))) {
    gnx_set_error("%s: T = %lld is not in -2^20..2^19 (a kinship of -1..0.5)", who, (long long)T);
    return 1;
  }
  if (max_pairs < 1 || max_pairs > (1ll << 26)) {
    gnx_set_error("%s: max_pairs must be in 1..2^26 (got %lld)", who, (long long)max_pairs);
    return 1;
  }
  if (!work || (max_work > 0 && (!n_candidates || !n_found || !pa || !pb || !hh || !ibs0 ||
                                 !nhet))) {
    gnx_set_error("%s: null work or output", who);
    return 1;
  }
  h->kin_ms = 0.0;
  h->kin_launches = h->kin_tasks = 0;
  std::vector<int32_t> widx;
  std::vector<u64> wmask;
  geno_words(h, locus_mask, widx, wmask);
  const int nw = (int)widx.size();
  const SgsGrid grid = sgs_grid(h, max_dist);
  const int all = std::isinf(grid.side) ? 1 : 0;

  GnxScratch s(who);
  int32_t* d_rows = nullptr;
  int64_t* d_slots = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows, &d_slots));
  const GnxSoA a = h->soa[h->cur];
  int32_t* d_order = nullptr;
  std::vector<int32_t> start;
  GnxCallTimer tm(h, &h->kin_ms, &h->kin_launches);
  tm.start();
  GNXCHK(sgs_sort_cells(h, s, grid, n, d_slots, &d_order, start));
  GNXCHK(tm.stop(3));
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
  h->kin_tasks = n_tasks;
  const int blocks = (int)std::min<int64_t>(std::max<int64_t>(n_tasks, 1), KIN_BLOCKS);
  // a tile reads 64 rows from its first: 64 zero rows behind the sample
  const int64_t n_pad = n + 64;
  // no more keepers than candidate pairs
  const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(max_pairs, cand));
  int32_t *d_rows_sorted = nullptr, *d_nh = nullptr, *d_nhet = nullptr, *d_lhh = nullptr,
          *d_lib = nullptr;
  float *d_xs = nullptr, *d_ys = nullptr;
  u64* d_key = nullptr;
  unsigned long long* d_cnt = nullptr;
  SgsTask* d_tasks = nullptr;
  GNXCHK(s.get(&d_rows_sorted, (size_t)n));
  GNXCHK(s.get(&d_xs, (size_t)n));
  GNXCHK(s.get(&d_ys, (size_t)n));
  GNXCHK(s.get(&d_nh, (size_t)n));
  GNXCHK(s.get(&d_nhet, (size_t)n));
  GNXCHK(s.get(&d_tasks, (size_t)n_tasks));
  GNXCHK(s.get(&d_cnt, 2));
  GNXCHK(s.get(&d_key, (size_t)cap));
  GNXCHK(s.get(&d_lhh, (size_t)cap));
  GNXCHK(s.get(&d_lib, (size_t)cap));
  if (n_tasks) GNXCHK(gnx_h2d(h, d_tasks, tasks.data(), (size_t)n_tasks * sizeof(SgsTask)));
  HIPCHK(hipMemsetAsync(d_cnt, 0, 2 * sizeof(unsigned long long), h->stream));
  GenoOperand op;
  GNXCHK(geno_operand(h, s, n_pad, widx, wmask, 0, &op));
  tm.start();
  hipLaunchKernelGGL(k_sgs_arrange, dim3(gnx_grid(n, 256)), dim3(256), 0, h->stream, n, d_order,
                     d_slots, (const int32_t*)nullptr, d_rows, a.x, a.y, d_rows_sorted, d_xs,
                     d_ys);
  geno_gather(h, d_rows_sorted, n, op);
  hipLaunchKernelGGL(k_kin_nhet, dim3(gnx_grid(n, 64)), dim3(64), 0, h->stream, n, nw, op.Wm,
                     op.X, d_order, d_nh, d_nhet);
  hipLaunchKernelGGL(k_kin_pairs, dim3(blocks), dim3(256), 0, h->stream, n_tasks, op.Wm, n,
                     d_tasks, op.X, d_xs, d_ys, d_nh, d_order, all, max_dist, (long long)T,
                     (unsigned long long)cap, d_cnt, d_key, d_lhh, d_lib);
  HIPCHK(hipGetLastError());
  GNXCHK(tm.stop(4));
  unsigned long long cnt[2] = {0, 0};
  GNXCHK(gnx_d2h(h, cnt, d_cnt, sizeof(cnt)));
  *n_found = (int64_t)cnt[0];
  if ((int64_t)cnt[0] > max_pairs) {
    gnx_set_error("%s: %lld kept pairs exceed max_pairs = %lld", who, (long long)cnt[0],
                  (long long)max_pairs);
    return 1;
  }
  *n_candidates = (int64_t)cnt[1];
  GNXCHK(gnx_d2h(h, nhet, d_nhet, (size_t)n * sizeof(int32_t)));
  const int64_t m = (int64_t)cnt[0];
  if (m == 0) return 0;
  u64* d_key2 = nullptr;
  int32_t *d_src = nullptr, *d_src2 = nullptr, *d_pa = nullptr, *d_pb = nullptr, *d_hh = nullptr,
          *d_ib = nullptr;
  char* d_tmp = nullptr;
  size_t tmp_bytes = 0;
  GNXCHK(gnx_prim_sort64_bytes((size_t)m, &tmp_bytes));
  GNXCHK(s.get(&d_key2, (size_t)m));
  GNXCHK(s.get(&d_src, (size_t)m));
  GNXCHK(s.get(&d_src2, (size_t)m));
  GNXCHK(s.get(&d_pa, (size_t)m));
  GNXCHK(s.get(&d_pb, (size_t)m));
  GNXCHK(s.get(&d_hh, (size_t)m));
  GNXCHK(s.get(&d_ib, (size_t)m));
  GNXCHK(s.get(&d_tmp, tmp_bytes));
  tm.start();
  hipLaunchKernelGGL(k_kin_iota, dim3(gnx_grid(m, 256)), dim3(256), 0, h->stream, m, d_src);
  GNXCHK(gnx_prim_sort64(d_tmp, tmp_bytes, (const uint64_t*)d_key, (uint64_t*)d_key2, d_src,
                         d_src2, (size_t)m, h->stream));
  hipLaunchKernelGGL(k_kin_emit, dim3(gnx_grid(m, 256)), dim3(256), 0, h->stream, m, n, d_key2,
                     d_src2, d_lhh, d_lib, d_pa, d_pb, d_hh, d_ib);
  HIPCHK(hipGetLastError());
  GNXCHK(tm.stop(3));
  GNXCHK(gnx_d2h(h, pa, d_pa, (size_t)m * sizeof(int32_t)));
  GNXCHK(gnx_d2h(h, pb, d_pb, (size_t)m * sizeof(int32_t)));
  GNXCHK(gnx_d2h(h, hh, d_hh, (size_t)m * sizeof(int32_t)));
  return gnx_d2h(h, ibs0, d_ib, (size_t)m * sizeof(int32_t));
}
