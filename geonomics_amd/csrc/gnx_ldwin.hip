// Windowed linkage disequilibrium on the device: for every locus of a request the number of
// kept loci within `window` of it and the sum of its r^2 with them, and the list of the pairs
// whose r^2 reaches r2_min - what LD pruning, clumping and LD scores are made of on the host
// (geonomics_amd/sim/ldwin.py).  include/gnx_ldwin.h says what is computed.
//
//   gnx_ld_window   c1, partners [n_loci] int64, score [n_loci] fp64, edges (ei, ej, er2), work
//
// The bit rows come from gnx_ld.hip's transpose (ld_transpose: k_ld_bits, k_ld_rowsum).  A task
// is a tile of 64 x 64 loci (i-tile <= j-tile) whose nearest pair is within the window; pos
// ascends, so the j-tiles of an i-tile are ti .. jhi[ti] - 1 and jhi ascends.  The loci are worked
// off in stretches of consecutive i-tiles t0 .. t1 - 1: ONE buffer holds the bit rows of tiles
// t0 .. jhi[t1 - 1] - 1, the stretch and the halo its windows reach, and the stretch is as long
// as that buffer and the tasks' partial sums fit the byte budget (gnx_ld_budget).
//
// k_ldw_pairs: the main loop is a copy of k_ld_pairs' LDS-staged popcount tile (gnx_ld.hip), not
// a shared function, so that kernel's code is untouched.  The epilogue takes the thread's
// sixteen pairs one at a time, rows outermost.  Row sums: the 64 columns of row ty + 16 r live in
// the 16 lanes that share ty; a lane adds its four in index order and an xor butterfly (8, 4, 2,
// 1) finishes.  Column sums: thread (tx, ty) owns the LDS slots [ty][tx + 16 c] and adds its four
// rows there in index order; after a barrier thread j adds the 16 slots of column j in ty order.
// Every task writes part[task][2][64] (int64 counts, fp64 sums); k_ldw_total, a thread per locus,
// adds the partials of the locus' tile to the running per-locus sums in task order.  The tasks
// are ordered by (ti, tj) whatever the stretches, so no output depends on the budget, and there
// are no floating-point atomics: a repeated call is bit-equal.
// Edges follow k_kin_pairs (gnx_kin.hip): a ballot of the qualifying lanes, one atomicAdd per
// wave for the space, the lanes' ranks from the ballot, keepers past the capacity counted but not
// written, then the list sorted by the key ei * n_loci + ej (gnx_prim_sort64) since the order
// of arrival is not fixed.
#include <cmath>
#include "gnx_geno.h"

#define LDW_K 16                  // chromosome words per LDS stage (= gnx_ld.hip's LD_K)
#define LDW_BLOCKS 2048           // workgroups of the pair kernel at most
#define LDW_BUDGET (256ll << 20)  // bytes resident unless gnx_ld_budget says so
#define LDW_MAX_CHROM (1ll << 26) // n c_ij - c_i c_j stays below 2^52: exact in fp64
#define LDW_PART_BYTES 1024       // a task's partials of one kind: [2][64] int64 or fp64
#define LDW_CP 80                 // pitch of the column slots: the two ty of a half-wave read other banks

struct alignas(16) LdwChunk {
  u64 a, b;
};

struct LdwTask {
  int32_t ti, tj;                 // tiles of 64 loci (indices into the request), ti <= tj
};

// see the head of the file.  T: the bit rows of tiles tb0 .. (row pitch `pitch` words, a multiple
// of LDW_K); n = the sampled chromosomes, mm = max(1, min_minor).  want_scores: part_i / part_f
// [n_tasks][2][64] (side 0: the loci of ti, side 1: of tj).  cap > 0: the edge list key / val
// [cap] behind counter[0]
__global__ void __launch_bounds__(256)
k_ldw_pairs(int64_t n_tasks, const LdwTask* __restrict__ tasks, int64_t pitch, int n_loci,
            const u64* __restrict__ T, int tb0, long long n, long long mm, double window,
            double r2_min, const long long* __restrict__ c1, const double* __restrict__ pos,
            int want_scores, long long* __restrict__ part_i, double* __restrict__ part_f,
            unsigned long long cap, unsigned long long* __restrict__ counter,
            u64* __restrict__ key, double* __restrict__ val) {
  __shared__ u64 AB[2][LDW_K][65];
  __shared__ long long cc[2][64];
  __shared__ double pp[2][64];
  u64 (*As)[65] = AB[0], (*Bs)[65] = AB[1];
  // the column slots take the stages' place: the main loop ends behind a barrier, and the next
  // task stages behind the one at its head
  static_assert(sizeof(AB) >= 16 * LDW_CP * (sizeof(double) + sizeof(int)), "column slots");
  double (*colf)[LDW_CP] = (double (*)[LDW_CP])&AB[0][0][0];
  int (*coli)[LDW_CP] = (int (*)[LDW_CP])(&AB[0][0][0] + 16 * LDW_CP);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63;
  const u64 below = (1ull << lane) - 1ull;
  for (int64_t t = blockIdx.x; t < n_tasks; t += gridDim.x) {
    const LdwTask K = tasks[t];
    __syncthreads();                                  // the last task's epilogue has read cc, pp
    if (tid < 128) {
      const int side = tid >> 6, i = tid & 63;
      const int64_t g = (int64_t)(side ? K.tj : K.ti) * 64 + i;
      cc[side][i] = g < n_loci ? c1[g] : 0;           // past the request: never kept
      pp[side][i] = g < n_loci ? pos[g] : 0.0;
    }
    const u64* a = T + (int64_t)(K.ti - tb0) * 64 * pitch;
    const u64* b = T + (int64_t)(K.tj - tb0) * 64 * pitch;
    int acc[4][4] = {};
    for (int64_t k0 = 0; k0 < pitch; k0 += LDW_K) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int q = tid + 256 * s;                  // (row, 16-byte chunk) with the chunk fastest
        const int row = q >> 3, c2 = (q & 7) * 2;
        const LdwChunk va = *(const LdwChunk*)(a + (int64_t)row * pitch + k0 + c2);
        const LdwChunk vb = *(const LdwChunk*)(b + (int64_t)row * pitch + k0 + c2);
        As[c2][row] = va.a;
        As[c2 + 1][row] = va.b;
        Bs[c2][row] = vb.a;
        Bs[c2 + 1][row] = vb.b;
      }
      __syncthreads();
#pragma unroll 4
      for (int kk = 0; kk < LDW_K; ++kk) {
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
    double rowf = 0.0;
    int rowc = 0;
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
      const bool in = min(ci, n - ci) >= mm && min(cj, n - cj) >= mm && (!diag || i < j) &&
                      d <= window;
      double r2 = 0.0;
      if (in) {
        const double dn = (double)(n * (long long)cij - ci * cj);
        r2 = (dn * dn) / ((double)(ci * (n - ci)) * (double)(cj * (n - cj)));
      }
      if (want_scores) {
        if (r == 0) {                                 // (wave-uniform: rc is)
          colf[ty][j] = r2;
          coli[ty][j] = in ? 1 : 0;
        } else {
          colf[ty][j] += r2;
          coli[ty][j] += in ? 1 : 0;
        }
        rowf = c == 0 ? r2 : rowf + r2;
        rowc = c == 0 ? (in ? 1 : 0) : rowc + (in ? 1 : 0);
        if (c == 3) {
          double f = rowf;
          int m = rowc;
#pragma unroll
          for (int s = 8; s > 0; s >>= 1) {
            f += __shfl_xor(f, s, 64);
            m += __shfl_xor(m, s, 64);
          }
          if (tx == 0) {
            part_f[(t * 2 + 0) * 64 + i] = f;
            part_i[(t * 2 + 0) * 64 + i] = m;
          }
        }
      }
      if (cap) {
        const bool keep = in && r2 >= r2_min;
        const u64 bal = __ballot(keep);
        if (bal == 0ull) continue;                    // wave-uniform
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(&counter[0], (unsigned long long)__popcll(bal));
        base = (unsigned long long)__shfl((long long)base, 0, 64);
        const unsigned long long k = base + (unsigned long long)__popcll(bal & below);
        if (keep && k < cap) {
          key[k] = (u64)((int64_t)K.ti * 64 + i) * (u64)n_loci + (u64)((int64_t)K.tj * 64 + j);
          val[k] = r2;
        }
      }
    }
    if (want_scores) {
      __syncthreads();                                // every thread's column slots are written
      if (tid < 64) {
        double f = 0.0;
        long long m = 0;
#pragma unroll
        for (int y = 0; y < 16; ++y) {
          f += colf[y][tid];
          m += coli[y][tid];
        }
        part_f[(t * 2 + 1) * 64 + tid] = f;
        part_i[(t * 2 + 1) * 64 + tid] = m;
      }
    }
  }
}

// the partials of one stretch (i-tiles t0 .. t1 - 1, tasks in (ti, tj) order from toff[t0]) added
// to the running sums of the loci of tiles t0 .. tb1 - 1 in task order: of tile t, the column
// side of (ti, t) for ti < t ascending, both sides of (t, t), the row side of (t, tj > t).
// toff[t] = the tasks before i-tile t, jhi as above, ilo[t] = the first i-tile that reaches t
__global__ void k_ldw_total(int n_loci, int t0, int t1, int tb1, const long long* __restrict__ toff,
                            const int32_t* __restrict__ jhi, const int32_t* __restrict__ ilo,
                            const long long* __restrict__ part_i,
                            const double* __restrict__ part_f, long long* __restrict__ partners,
                            double* __restrict__ score) {
  const int64_t g = (int64_t)t0 * 64 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_loci || g >= (int64_t)tb1 * 64) return;
  const int t = (int)(g >> 6), l = (int)(g & 63);
  long long m = partners[g];
  double s = score[g];
  const long long base = toff[t0];
  for (int ti = max(t0, ilo[t]); ti < min(t, t1); ++ti) {
    const long long k = toff[ti] - base + (t - ti);
    m += part_i[(k * 2 + 1) * 64 + l];
    s += part_f[(k * 2 + 1) * 64 + l];
  }
  if (t < t1) {
    const long long k0 = toff[t] - base;
    const int nj = jhi[t] - t;
    for (int q = 0; q < nj; ++q) {
      m += part_i[((k0 + q) * 2 + 0) * 64 + l];
      s += part_f[((k0 + q) * 2 + 0) * 64 + l];
      if (q == 0) {
        m += part_i[(k0 * 2 + 1) * 64 + l];
        s += part_f[(k0 * 2 + 1) * 64 + l];
      }
    }
  }
  partners[g] = m;
  score[g] = s;
}

__global__ void k_ldw_iota(int64_t m, int32_t* __restrict__ v) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < m) v[k] = (int32_t)k;
}

// the sorted list: entry k is (key[k] / n_loci, key[k] % n_loci) with the r^2 of list entry src[k]
__global__ void k_ldw_emit(int64_t m, int64_t n_loci, const u64* __restrict__ key,
                           const int32_t* __restrict__ src, const double* __restrict__ val,
                           int32_t* __restrict__ ei, int32_t* __restrict__ ej,
                           double* __restrict__ er2) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const u64 a = key[k] / (u64)n_loci;
  ei[k] = (int32_t)a;
  ej[k] = (int32_t)(key[k] - a * (u64)n_loci);
  er2[k] = val[src[k]];
}

extern "C" int gnx_ld_window_info(gnx_state* h, double* kernel_ms, int64_t* launches,
                                  int64_t* locus_blocks) {
  if (kernel_ms) *kernel_ms = h->ldw_ms;
  if (launches) *launches = h->ldw_launches;
  if (locus_blocks) *locus_blocks = h->ldw_blocks;
  return 0;
}

extern "C" int gnx_ld_window(gnx_state* h, int64_t n, const int64_t* slots, int32_t n_loci,
                             const int32_t* loci, const double* pos, double window,
                             int32_t min_minor, double r2_min, int64_t max_edges,
                             int64_t max_work, int64_t* work, int64_t* c1, int64_t* partners,
                             double* score, int64_t* n_edges, int32_t* ei, int32_t* ej,
                             double* er2) {
  const char* who = "gnx_ld_window";
  h->ldw_ms = 0.0;
  h->ldw_launches = 0;
  h->ldw_blocks = 0;
  GNXCHK(geno_ready(h, who));
  if (n < 1 || 2 * n > LDW_MAX_CHROM) {
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
  if (std::isnan(window) || window < 0.0) {
    gnx_set_error("%s: window must be >= 0 (it may be +inf) (got %g)", who, window);
    return 1;
  }
  if (!(r2_min >= 0.0 && r2_min <= 1.0)) {
    gnx_set_error("%s: r2_min must be in 0..1 (got %g)", who, r2_min);
    return 1;
  }
  if (max_edges < 0 || max_edges > (1ll << 26)) {
    gnx_set_error("%s: max_edges must be in 0..2^26 (got %lld)", who, (long long)max_edges);
    return 1;
  }
  if (!work || (max_work > 0 && (!c1 || (max_edges > 0 && (!n_edges || !ei || !ej || !er2))))) {
    gnx_set_error("%s: null work or output", who);
    return 1;
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
  // ---- the tiles whose nearest pair is within the window: of i-tile ti, tiles ti .. jhi - 1
  const int64_t n_chrom = 2 * n;
  const int64_t nq = (n_chrom + 63) / 64;
  const int64_t pitch = (nq + LDW_K - 1) / LDW_K * LDW_K;
  const int nt = (n_loci + 63) / 64;
  auto first_of = [&](int t) { return pos[(size_t)t * 64]; };
  auto last_of = [&](int t) { return pos[std::min<size_t>((size_t)t * 64 + 63, (size_t)n_loci - 1)]; };
  std::vector<int32_t> jhi((size_t)nt), ilo((size_t)nt);
  std::vector<long long> toff((size_t)nt + 1, 0);
  for (int ti = 0, tj = 0; ti < nt; ++ti) {           // (jhi ascends with ti: tj is not reset)
    tj = std::max(tj, ti + 1);
    while (tj < nt && first_of(tj) - last_of(ti) <= window) ++tj;
    jhi[(size_t)ti] = tj;
    toff[(size_t)ti + 1] = toff[(size_t)ti] + (tj - ti);
  }
  for (int t = 0, ti = 0; t < nt; ++t) {
    while (jhi[(size_t)ti] <= t) ++ti;                // (jhi[t] > t ends it)
    ilo[(size_t)t] = ti;
  }
  const int64_t n_listed = toff[(size_t)nt];
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
  // ---- stretches of i-tiles: the buffer (stretch and halo) and the partials under the budget
  const int64_t budget = h->ld_budget > 0 ? h->ld_budget : LDW_BUDGET;
  const int64_t tile_bytes = 64 * pitch * 8;
  const bool want_scores = partners || score;
  const int64_t part_bytes = want_scores ? 2 * LDW_PART_BYTES : 0;
  std::vector<std::pair<int, int>> blocks;
  int64_t max_tiles = 1, max_tasks = 1;
  for (int t0 = 0; t0 < nt;) {
    int t1 = t0;
    int64_t tasks = 0;
    while (t1 < nt) {
      const int64_t more = tasks + (jhi[(size_t)t1] - t1);
      const int64_t bytes = (int64_t)(jhi[(size_t)t1] - t0) * tile_bytes + more * part_bytes;
      if (bytes > budget) break;
      tasks = more;
      ++t1;
    }
    if (t1 == t0) {
      const int64_t reach = jhi[(size_t)t0] - t0;
      gnx_set_error("%s: tile %d of 64 loci and the %lld tiles its window reaches take %lld "
                    "bytes of bit rows and partial sums, above the budget of %lld bytes "
                    "(gnx_ld_budget)", who, t0, (long long)(reach - 1),
                    (long long)(reach * (tile_bytes + part_bytes)), (long long)budget);
      return 1;
    }
    blocks.push_back({t0, t1});
    max_tiles = std::max<int64_t>(max_tiles, jhi[(size_t)t1 - 1] - t0);
    max_tasks = std::max(max_tasks, tasks);
    t0 = t1;
  }
  h->ldw_blocks = (int64_t)blocks.size();

  GnxScratch s(who);
  int32_t* d_rows = nullptr;
  GNXCHK(geno_rows(h, who, n, slots, s, &d_rows));
  const int64_t buf_words = max_tiles * 64 * pitch;
  const unsigned long long cap = (unsigned long long)max_edges;
  u64 *T = nullptr, *d_key = nullptr;
  int32_t *d_jof = nullptr, *d_lines = nullptr, *d_jhi = nullptr, *d_ilo = nullptr;
  long long *d_c1 = nullptr, *d_toff = nullptr, *d_pi = nullptr, *d_partners = nullptr;
  double *d_pos = nullptr, *d_pf = nullptr, *d_score = nullptr, *d_val = nullptr;
  unsigned long long* d_cnt = nullptr;
  LdwTask* d_tasks = nullptr;
  GNXCHK(s.get(&T, (size_t)buf_words));
  GNXCHK(s.get(&d_jof, jof.size()));
  GNXCHK(s.get(&d_lines, (size_t)std::min<int64_t>(n_loci, max_tiles * 64)));
  GNXCHK(s.get(&d_c1, (size_t)n_loci));
  GNXCHK(s.get(&d_pos, (size_t)n_loci));
  GNXCHK(s.get(&d_tasks, (size_t)max_tasks));
  GNXCHK(s.get(&d_cnt, 1));
  GNXCHK(s.get(&d_key, (size_t)cap));
  GNXCHK(s.get(&d_val, (size_t)cap));
  if (want_scores) {
    GNXCHK(s.get(&d_jhi, (size_t)nt));
    GNXCHK(s.get(&d_ilo, (size_t)nt));
    GNXCHK(s.get(&d_toff, (size_t)nt + 1));
    GNXCHK(s.get(&d_pi, (size_t)max_tasks * 128));
    GNXCHK(s.get(&d_pf, (size_t)max_tasks * 128));
    GNXCHK(s.get(&d_partners, (size_t)n_loci));
    GNXCHK(s.get(&d_score, (size_t)n_loci));
    GNXCHK(gnx_h2d(h, d_jhi, jhi.data(), (size_t)nt * sizeof(int32_t)));
    GNXCHK(gnx_h2d(h, d_ilo, ilo.data(), (size_t)nt * sizeof(int32_t)));
    GNXCHK(gnx_h2d(h, d_toff, toff.data(), ((size_t)nt + 1) * sizeof(long long)));
    HIPCHK(hipMemsetAsync(d_partners, 0, (size_t)n_loci * sizeof(long long), h->stream));
    HIPCHK(hipMemsetAsync(d_score, 0, (size_t)n_loci * sizeof(double), h->stream));
  }
  GNXCHK(gnx_h2d(h, d_jof, jof.data(), jof.size() * sizeof(int32_t)));
  GNXCHK(gnx_h2d(h, d_pos, pos, (size_t)n_loci * sizeof(double)));
  HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), h->stream));
  HIPCHK(hipMemsetAsync(d_c1, 0, (size_t)n_loci * sizeof(long long), h->stream));

  const long long mm = std::max<long long>(1, min_minor);
  std::vector<LdwTask> tasks;
  std::vector<int32_t> lines;
  GnxCallTimer tm(h, &h->ldw_ms, &h->ldw_launches);
  for (const auto& bk : blocks) {
    const int t0 = bk.first, t1 = bk.second, tb1 = jhi[(size_t)t1 - 1];
    const int ja = t0 * 64, nj = (int)std::min<int64_t>(n_loci, (int64_t)tb1 * 64) - ja;
    tasks.clear();
    for (int ti = t0; ti < t1; ++ti)
      for (int tj = ti; tj < jhi[(size_t)ti]; ++tj) tasks.push_back(LdwTask{ti, tj});
    lines.clear();
    for (int j = ja; j < ja + nj; ++j) lines.push_back(loci[j] >> 10);
    std::sort(lines.begin(), lines.end());
    lines.erase(std::unique(lines.begin(), lines.end()), lines.end());
    GNXCHK(gnx_h2d(h, d_tasks, tasks.data(), tasks.size() * sizeof(LdwTask)));
    GNXCHK(gnx_h2d(h, d_lines, lines.data(), lines.size() * sizeof(int32_t)));
    tm.start();
    int64_t launches = ld_transpose(h, n_chrom, nq, pitch, (int)lines.size(), d_lines, d_rows,
                                    d_jof, ja, nj, T, buf_words, d_c1 + ja);
    hipLaunchKernelGGL(k_ldw_pairs, dim3((unsigned)std::min<int64_t>((int64_t)tasks.size(),
                                                                      LDW_BLOCKS)),
                       dim3(256), 0, h->stream, (int64_t)tasks.size(), d_tasks, pitch, (int)n_loci,
                       T, t0, (long long)n_chrom, mm, window, r2_min, d_c1, d_pos,
                       (int)want_scores, d_pi, d_pf, cap, d_cnt, d_key, d_val);
    ++launches;
    if (want_scores) {
      hipLaunchKernelGGL(k_ldw_total, dim3(gnx_grid(nj, 256)), dim3(256), 0, h->stream,
                         (int)n_loci, t0, t1, tb1, d_toff, d_jhi, d_ilo, d_pi, d_pf, d_partners,
                         d_score);
      ++launches;
    }
    HIPCHK(hipGetLastError());
    GNXCHK(tm.stop(launches));
  }
  unsigned long long cnt = 0;
  if (max_edges > 0) {
    GNXCHK(gnx_d2h(h, &cnt, d_cnt, sizeof(cnt)));
    *n_edges = (int64_t)cnt;
    if ((int64_t)cnt > max_edges) {
      gnx_set_error("%s: %lld pairs with r2 >= %g exceed max_edges = %lld", who, (long long)cnt,
                    r2_min, (long long)max_edges);
      return 1;
    }
  }
  std::vector<long long> c1h((size_t)n_loci);
  GNXCHK(gnx_d2h(h, c1h.data(), d_c1, c1h.size() * sizeof(long long)));
  for (int j = 0; j < n_loci; ++j) c1[j] = c1h[(size_t)j];
  if (partners) {
    GNXCHK(gnx_d2h(h, c1h.data(), d_partners, c1h.size() * sizeof(long long)));
    for (int j = 0; j < n_loci; ++j) partners[j] = c1h[(size_t)j];
  }
  if (score) GNXCHK(gnx_d2h(h, score, d_score, (size_t)n_loci * sizeof(double)));
  const int64_t m = (int64_t)cnt;
  if (m == 0) return 0;
  u64* d_key2 = nullptr;
  int32_t *d_src = nullptr, *d_src2 = nullptr, *d_ei = nullptr, *d_ej = nullptr;
  double* d_er2 = nullptr;
  char* d_tmp = nullptr;
  size_t tmp_bytes = 0;
  GNXCHK(gnx_prim_sort64_bytes((size_t)m, &tmp_bytes));
  GNXCHK(s.get(&d_key2, (size_t)m));
  GNXCHK(s.get(&d_src, (size_t)m));
  GNXCHK(s.get(&d_src2, (size_t)m));
  GNXCHK(s.get(&d_ei, (size_t)m));
  GNXCHK(s.get(&d_ej, (size_t)m));
  GNXCHK(s.get(&d_er2, (size_t)m));
  GNXCHK(s.get(&d_tmp, tmp_bytes));
  tm.start();
  hipLaunchKernelGGL(k_ldw_iota, dim3(gnx_grid(m, 256)), dim3(256), 0, h->stream, m, d_src);
  GNXCHK(gnx_prim_sort64(d_tmp, tmp_bytes, (const uint64_t*)d_key, (uint64_t*)d_key2, d_src,
                         d_src2, (size_t)m, h->stream));
  hipLaunchKernelGGL(k_ldw_emit, dim3(gnx_grid(m, 256)), dim3(256), 0, h->stream, m,
                     (int64_t)n_loci, d_key2, d_src2, d_val, d_ei, d_ej, d_er2);
  HIPCHK(hipGetLastError());
  GNXCHK(tm.stop(3));
  GNXCHK(gnx_d2h(h, ei, d_ei, (size_t)m * sizeof(int32_t)));
  GNXCHK(gnx_d2h(h, ej, d_ej, (size_t)m * sizeof(int32_t)));
  return gnx_d2h(h, er2, d_er2, (size_t)m * sizeof(double));
}
